// test_regression_data.cpp -- the reference's Test_Regression driver end to end (Test_Regression.cpp:10-67), with NUMBERS in and NUMBERS out:
//
//   test_regression_data p generator dim nrows datafile [seed] [--devices=0,0] [--literal]
//
// writes a seeded data file in the reference's format ("dim n", then n rows of dim integers and a label), then runs
//   LoadData -> BatchData -> AddDataSlots -> RegressBatched (masked with GenerateNoise) -> DecryptSlotsBatch -> slot 0
// and compares slot 0 of theta[i] and det with the integer regression adj(X^T X) X^T y and det(X^T X) taken modulo p (RegressPT,
// Regression.h:193-217, computed here with exact integers).  Context as in Test_Regression.cpp:85-125: m = p - 1, logQ from the same formula.
// --devices runs the waves once more sharded over that group (a repeated GPU gives a loopback group); --literal once through the
// object-at-a-time evaluator (matrix_literal.h).  Exit code 0 on success.
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>

#include "matrix_literal.h"

using namespace fhesi;
namespace fhesi { FHEcontext* activeContext = nullptr; }

typedef __int128 wide;
static long mod_p(wide v, long p) { long r = (long)(v % p); return r < 0 ? r + p : r; }
// determinant by Laplace expansion along the first row (d <= 4 here)
static wide det_of(const std::vector<std::vector<wide>>& A) {
  const size_t d = A.size();
  if (d == 1) return A[0][0];
  wide s = 0;
  for (size_t c = 0; c < d; ++c) {
    std::vector<std::vector<wide>> M;
    for (size_t i = 1; i < d; ++i) { std::vector<wide> row; for (size_t j = 0; j < d; ++j) if (j != c) row.push_back(A[i][j]); M.push_back(row); }
    s += (c % 2 ? -1 : 1) * A[0][c] * det_of(M);
  }
  return s;
}
static wide cofactor(const std::vector<std::vector<wide>>& A, size_t r, size_t c) {
  std::vector<std::vector<wide>> M;
  for (size_t i = 0; i < A.size(); ++i) { if (i == r) continue; std::vector<wide> row; for (size_t j = 0; j < A.size(); ++j) if (j != c) row.push_back(A[i][j]); M.push_back(row); }
  return ((r + c) % 2 ? -1 : 1) * det_of(M);
}

int main(int argc, char* argv[]) {
  std::vector<int> devices; bool literal = false;
  std::vector<char*> args;
  for (int i = 1; i < argc; ++i) {
    if (!strncmp(argv[i], "--devices=", 10)) { for (char* t = strtok(argv[i] + 10, ","); t; t = strtok(nullptr, ",")) devices.push_back(atoi(t)); }
    else if (!strcmp(argv[i], "--literal")) literal = true;
    else args.push_back(argv[i]);
  }
  if (args.size() < 5) { std::cout << "usage: test_regression_data p generator dim nrows datafile [seed] [--devices=0,0] [--literal]" << std::endl; return 1; }
  const unsigned p = atoi(args[0]), g = atoi(args[1]), dimArg = atoi(args[2]), nrows = atoi(args[3]);
  const std::string datafile = args[4];
  const long long seed = args.size() >= 6 ? atoll(args[5]) : 1;

  {   // the data file, seeded: small non-negative features and labels, as scripts/generateRandomData.py writes them
    SetSeed((uint64_t)seed * 7919);
    std::ofstream out(datafile);
    out << dimArg << " " << nrows << "\n";
    for (unsigned i = 0; i < nrows; ++i) { for (unsigned j = 0; j <= dimArg; ++j) out << RandomBnd(10L) << (j == dimArg ? "\n" : " "); }
  }
  Matrix<ZZ> rawData; std::vector<ZZ> labels; unsigned dim = 0;
  if (!LoadData(rawData, labels, dim, datafile) || dim != dimArg || rawData.NumRows() != nrows) { std::cout << "LoadData failed" << std::endl; return 1; }

  // RegressPT with exact integers
  std::vector<std::vector<wide>> A(dim, std::vector<wide>(dim, 0)); std::vector<wide> b(dim, 0);
  for (unsigned i = 0; i < nrows; ++i)
    for (unsigned a = 0; a < dim; ++a) { b[a] += (wide)rawData(i, a).to_long() * labels[i].to_long(); for (unsigned c = 0; c < dim; ++c) A[a][c] += (wide)rawData(i, a).to_long() * rawData(i, c).to_long(); }
  std::vector<long> thetaE(dim); long detE;
  if (dim == 1) { detE = mod_p(A[0][0], p); thetaE[0] = mod_p(b[0], p); }
  else {
    detE = mod_p(det_of(A), p);
    for (unsigned i = 0; i < dim; ++i) { wide s = 0; for (unsigned k = 0; k < dim; ++k) s += cofactor(A, k, i) * b[k]; thetaE[i] = mod_p(s, p); }      // adj(i,k) = cofactor(k,i)
  }
  std::cout << "Expected values:" << std::endl;
  for (unsigned i = 0; i < dim; ++i) std::cout << "  theta[" << i << "] = " << thetaE[i] << std::endl;
  std::cout << "  Determinant: " << detE << std::endl;

  // Test_Regression.cpp:85-108
  unsigned blockSize = 1; { unsigned val = (p - 1) / 2 - 1; while (val > 1) { blockSize <<= 1; val >>= 1; } }
  const unsigned n = (p - 1) / 2 - 1, nBlocks = (nrows + blockSize - 1) / blockSize, xi = std::max(nBlocks, dim);
  const double lgQ = 4.5 * std::log((double)n) + std::max(1, (int)dim - 1) * (std::log(1280.0) + 2 * std::log((double)n) + std::log((double)xi));
  const unsigned logQ = (unsigned)std::ceil(lgQ / std::log(2.0) + 24.7);
  FHEcontext context(p - 1, logQ, p, g, 3);
  activeContext = &context;
  context.SetUpSIContext(xi);
  const PlaintextSpace& space = context.GetPlaintextSpace();
  std::cout << "regression on data: p=" << p << " m=" << p - 1 << " slots=" << space.GetTotalSlots() << " usable=" << space.GetUsableSlots() << " logQ=" << logQ
            << " dim=" << dim << " rows=" << nrows << " blocks=" << nBlocks << std::endl;
  int failures = 0;
  auto expect = [&](bool ok, const char* what) { std::cout << what << ": " << (ok ? "yes" : "NO") << std::endl; if (!ok) ++failures; };

  // BatchData: one device embed for the whole data set; the plaintexts decode to the columns of their block
  std::vector<std::vector<Plaintext>> ptxtData; std::vector<Plaintext> ptxtLabels;
  BatchData(ptxtData, ptxtLabels, rawData, labels, context);
  {
    bool ok = ptxtData.size() == nBlocks && ptxtLabels.size() == nBlocks;
    for (unsigned blk = 0; ok && blk < nBlocks; ++blk) {
      std::vector<long> slots; ptxtData[blk][dim - 1].DecodeSlots(slots);
      ok = slots.size() == space.GetTotalSlots();
      for (unsigned k = 0; ok && k < space.GetUsableSlots(); ++k) { const unsigned row = blk * space.GetUsableSlots() + k; ok = slots[k] == (row < nrows ? rawData(row, dim - 1).to_long() % (long)p : 0); }
      long v = -1; ptxtLabels[blk].DecodeSlot(v, 0); ok = ok && v == labels[blk * space.GetUsableSlots()].to_long() % (long)p;
    }
    expect(ok, "BatchData plaintexts decode to the data");
    // Plaintext >>= 1 moves slot j + 1 into slot j; += and == act on the message
    Plaintext a = ptxtData[0][0], r = a; r >>= 1;
    std::vector<long> sa, sr; a.DecodeSlots(sa, false); r.DecodeSlots(sr, false);
    bool rot = true; for (size_t j = 0; j < sa.size(); ++j) rot = rot && sr[j] == sa[(j + 1) % sa.size()];
    Plaintext sum = a; sum += r; sum -= r;
    expect(rot && sum == a && !(r == a), "Plaintext >>= 1 rotates left by one, += / -= / == hold");
  }

  SetSeed((uint64_t)seed);
  Regression regress(context);
  SeedSequence seq((uint64_t)seed * 0x9e3779b97f4a7c15ull + 1, (uint64_t)seed * 0xbf58476d1ce4e5b9ull + 2);
  regress.AddDataSlots(rawData, labels, seq);

  auto slot0 = [&](const char* what, std::vector<Ciphertext> theta, const Ciphertext& det, std::vector<std::vector<long>>* all = nullptr) {
    theta.push_back(det);
    std::vector<std::vector<long>> vals;
    regress.GetSecretKey().DecryptSlotsBatch(vals, theta, 0, false);
    std::cout << "Computed values (" << what << "):" << std::endl;
    bool ok = true;
    for (unsigned i = 0; i < dim; ++i) { std::cout << "  theta[" << i << "] = " << vals[i][0] << std::endl; ok = ok && vals[i][0] == thetaE[i]; }
    std::cout << "  Determinant: " << vals[dim][0] << std::endl;
    ok = ok && vals[dim][0] == detE;
    expect(ok, (std::string(what) + ": slot 0 equals the integer regression modulo p").c_str());
    if (all) *all = vals;
  };

  std::vector<Ciphertext> thetaU, thetaM; Ciphertext detU(context), detM(context);
  std::vector<std::vector<long>> plainU, plainM;
  regress.RegressBatched(thetaU, detU);
  slot0("batched, unmasked", thetaU, detU, &plainU);
  regress.RegressBatched(thetaM, detM, seq);
  slot0("batched, masked", thetaM, detM, &plainM);
  if (dim > 1) {
    long changed = 0, slots = 0;
    for (size_t i = 0; i < plainM.size(); ++i) for (size_t j = 1; j < plainM[i].size(); ++j) { ++slots; changed += plainM[i][j] != plainU[i][j]; }
    std::cout << "masked slots that differ from the unmasked partial sums: " << changed << " of " << slots << std::endl;
    expect(changed * 10 > slots * 9, "the masks replace the other slots");
  }
  if (!devices.empty()) {
    std::vector<Ciphertext> thetaG; Ciphertext detG(context);
    regress.RegressBatchedMultiGpu(devices, thetaG, detG, 1, &seq);
    slot0("group of ranks, masked", thetaG, detG);
  }
  if (literal) {
    std::vector<Ciphertext> thetaL; Ciphertext detL(context);
    RegressLiteral(regress, thetaL, detL);
    regress.AddNoise(thetaL, detL, seq);
    slot0("object at a time, masked", thetaL, detL);
  }
  std::cout << (failures ? "FAILED" : "OK") << std::endl;
  return failures ? 1 : 0;
}
