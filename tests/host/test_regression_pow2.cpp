// test_regression_pow2.cpp -- the data-file regression driver of test_regression_data.cpp on a POWER-OF-TWO ring, where the slots form two rows
// (m = 2^k, p = 1 mod m; include/fhesi_hip.h, "the TWO-ROW space"):
//
//   test_regression_pow2 m p generator dim nrows datafile [seed] [--devices=0,0]        dim = 1 or 2
//
// writes a seeded data file ("dim n", then n rows of dim integers and a label), then runs
//   LoadData -> BatchData -> AddDataSlots -> RegressBatched (unmasked, and masked with GenerateNoise) -> DecryptSlotsBatch
// and compares slot 0 of theta[i] and det with the integer regression adj(X^T X) X^T y and det(X^T X) modulo p.  On the way it checks what is
// particular to these rings: Rows() / Cols(), Plaintext >>= rotating each row, SwapRows, the exponent list g, g^2, ..., g^(n/4), m - 1 of
// Regression, and that the unmasked results carry the total in EVERY slot.  m / 2 slots per ciphertext, all usable.  Exit code 0 on success.
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>

#include "../../fhe-si_amd/host/fhesi_matrix.h"

using namespace fhesi;
namespace fhesi { FHEcontext* activeContext = nullptr; }

typedef __int128 wide;
static long mod_p(wide v, long p) { long r = (long)(v % p); return r < 0 ? r + p : r; }

int main(int argc, char* argv[]) {
  std::vector<int> devices;
  std::vector<char*> args;
  for (int i = 1; i < argc; ++i) {
    if (!strncmp(argv[i], "--devices=", 10)) { for (char* t = strtok(argv[i] + 10, ","); t; t = strtok(nullptr, ",")) devices.push_back(atoi(t)); }
    else args.push_back(argv[i]);
  }
  if (args.size() < 6) { std::cout << "usage: test_regression_pow2 m p generator dim nrows datafile [seed] [--devices=0,0]" << std::endl; return 1; }
  const unsigned m = atoi(args[0]), p = atoi(args[1]), g = atoi(args[2]), dimArg = atoi(args[3]), nrows = atoi(args[4]);
  const std::string datafile = args[5];
  const long long seed = args.size() >= 7 ? atoll(args[6]) : 1;
  if (dimArg < 1 || dimArg > 2) { std::cout << "dim must be 1 or 2" << std::endl; return 1; }

  {
    SetSeed((uint64_t)seed * 7919);
    std::ofstream out(datafile);
    out << dimArg << " " << nrows << "\n";
    for (unsigned i = 0; i < nrows; ++i) { for (unsigned j = 0; j <= dimArg; ++j) out << RandomBnd(10L) << (j == dimArg ? "\n" : " "); }
  }
  Matrix<ZZ> rawData; std::vector<ZZ> labels; unsigned dim = 0;
  if (!LoadData(rawData, labels, dim, datafile) || dim != dimArg || rawData.NumRows() != nrows) { std::cout << "LoadData failed" << std::endl; return 1; }

  // the plaintext regression with exact integers: A = X^T X, b = X^T y;  theta = adj(A) b, det = det(A)
  wide A[2][2] = {{0, 0}, {0, 0}}, b[2] = {0, 0};
  for (unsigned i = 0; i < nrows; ++i)
    for (unsigned a = 0; a < dim; ++a) { b[a] += (wide)rawData(i, a).to_long() * labels[i].to_long(); for (unsigned c = 0; c < dim; ++c) A[a][c] += (wide)rawData(i, a).to_long() * rawData(i, c).to_long(); }
  std::vector<long> thetaE(dim); long detE;
  if (dim == 1) { detE = mod_p(A[0][0], p); thetaE[0] = mod_p(b[0], p); }
  else {
    detE = mod_p(A[0][0] * A[1][1] - A[0][1] * A[1][0], p);
    thetaE[0] = mod_p(A[1][1] * b[0] - A[0][1] * b[1], p);
    thetaE[1] = mod_p(A[0][0] * b[1] - A[1][0] * b[0], p);
  }
  std::cout << "Expected values:" << std::endl;
  for (unsigned i = 0; i < dim; ++i) std::cout << "  theta[" << i << "] = " << thetaE[i] << std::endl;
  std::cout << "  Determinant: " << detE << std::endl;

  // one multiplication level per dimension on top of the inner products; p and the m / 2 slots both enter the noise of a level
  const unsigned nSlots = m / 2, nBlocks = (nrows + nSlots - 1) / nSlots, xi = std::max(nBlocks, dim), logQ = 100 + 100 * dim;
  FHEcontext context(m, logQ, p, g, 3);
  activeContext = &context;
  context.SetUpSIContext(xi);
  const PlaintextSpace& space = context.GetPlaintextSpace();
  std::cout << "regression on data: p=" << p << " m=" << m << " slots=" << space.GetTotalSlots() << " usable=" << space.GetUsableSlots() << " rows=" << space.Rows()
            << " cols=" << space.Cols() << " logQ=" << logQ << " dim=" << dim << " data rows=" << nrows << " blocks=" << nBlocks << std::endl;
  int failures = 0;
  auto expect = [&](bool ok, const char* what) { std::cout << what << ": " << (ok ? "yes" : "NO") << std::endl; if (!ok) ++failures; };
  expect(space.Rows() == 2 && space.Cols() == m / 4 && space.GetTotalSlots() == nSlots && space.GetUsableSlots() == nSlots, "two rows of m / 4 columns, every slot usable");

  std::vector<std::vector<Plaintext>> ptxtData; std::vector<Plaintext> ptxtLabels;
  BatchData(ptxtData, ptxtLabels, rawData, labels, context);
  {
    bool ok = ptxtData.size() == nBlocks && ptxtLabels.size() == nBlocks;
    for (unsigned blk = 0; ok && blk < nBlocks; ++blk) {
      std::vector<long> slots; ptxtData[blk][dim - 1].DecodeSlots(slots);
      ok = slots.size() == nSlots;
      for (unsigned k = 0; ok && k < nSlots; ++k) { const unsigned row = blk * nSlots + k; ok = slots[k] == (row < nrows ? rawData(row, dim - 1).to_long() % (long)p : 0); }
      long v = -1; ptxtLabels[blk].DecodeSlot(v, 0); ok = ok && v == labels[blk * nSlots].to_long() % (long)p;
    }
    expect(ok, "BatchData plaintexts decode to the data");
    // Plaintext >>= 3 rotates each row left by three columns; SwapRows exchanges the rows; the coefficient side agrees with X -> X^(m-1)
    const long h = (long)space.Cols();
    Plaintext a = ptxtData[0][0], r = a, s = a; r >>= 3; s.SwapRows();
    std::vector<long> sa, sr, ss; a.DecodeSlots(sa, false); r.DecodeSlots(sr, false); s.DecodeSlots(ss, false);
    bool rot = true, swp = true;
    for (long row = 0; row < 2; ++row) for (long j = 0; j < h; ++j) { rot = rot && sr[row * h + j] == sa[row * h + (j + 3) % h]; swp = swp && ss[row * h + j] == sa[(1 - row) * h + j]; }
    std::vector<long> conj(nSlots, 0);               // a(X^(m-1)) = a(X^-1) modulo X^n + 1: a_0, then -a_(n-i)
    for (unsigned i = 0; i < nSlots && i < a.message.size(); ++i) { if (!i) conj[0] = a.message[0]; else conj[nSlots - i] = (long)((p - a.message[i]) % p); }
    Plaintext c(context); c.message = conj;
    Plaintext sum = a; sum += r; sum -= r;
    expect(rot && sum == a && !(r == a), "Plaintext >>= 3 rotates both rows left by three, += / -= / == hold");
    expect(swp && c == s, "SwapRows exchanges the rows and equals X -> X^(m-1) on the coefficients");
  }

  SetSeed((uint64_t)seed);
  Regression regress(context);
  {
    const std::vector<unsigned>& ks = regress.AutomorphismExponents();
    unsigned lg = 0; while ((1u << lg) < nSlots) ++lg;
    bool ok = ks.size() == lg && ks.back() == m - 1 && ks[0] == g % m;
    for (size_t i = 0; ok && i + 1 < ks.size(); ++i) ok = ks[i] != 1 && (i == 0 || ks[i] == (unsigned)(((unsigned long)ks[i - 1] * ks[i - 1]) % m));
    expect(ok, "the exponents of the total sum are g, g^2, g^4, ..., then m - 1");
  }
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
  {
    bool same = true;
    for (auto& v : plainU) { same = same && v.size() == nSlots; for (long x : v) same = same && x == v[0]; }
    expect(same, "unmasked: the total reaches every slot of both rows");
  }
  regress.RegressBatched(thetaM, detM, seq);
  slot0("batched, masked", thetaM, detM, &plainM);
  if (dim > 1) {                                     // (d = 1 has no minors to hide: Regress returns the two sums as they are)
    long changed = 0, slots = 0;
    for (size_t i = 0; i < plainM.size(); ++i) for (size_t j = 1; j < plainM[i].size(); ++j) { ++slots; changed += plainM[i][j] != plainU[i][j]; }
    std::cout << "masked slots that differ from the unmasked ones: " << changed << " of " << slots << std::endl;
    expect(changed * 10 > slots * 9, "the masks replace the other slots");
  }
  if (!devices.empty()) {
    std::vector<Ciphertext> thetaG; Ciphertext detG(context);
    regress.RegressBatchedMultiGpu(devices, thetaG, detG, 1, &seq);
    slot0("group of ranks, masked", thetaG, detG);
  }
  std::cout << (failures ? "FAILED" : "OK") << std::endl;
  return failures ? 1 : 0;
}
