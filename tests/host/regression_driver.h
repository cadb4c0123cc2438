// regression_driver.h -- TEST HARNESS: what the data-file regression programs share (test_regression_data.cpp on the cyclic rings of the
// reference's driver, test_regression_pow2.cpp on the two-row rings): the command line, the seeded data file in the reference's format
// ("dim n", then n rows of dim integers and a label), the integer regression adj(X^T X) X^T y and det(X^T X) modulo p (RegressPT,
// Regression.h:193-217, computed here with exact integers), and the runs
//   RegressBatched (unmasked, and masked with GenerateNoise) [-> a group of ranks] [-> object at a time] -> DecryptSlotsBatch -> slot 0.
// Each program keeps what is particular to its ring: the context, the checks on BatchData and Plaintext, what the other slots hold.
#pragma once
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

struct RegressionDriver {
  std::vector<int> devices; bool literal = false;      // --devices=0,0: the waves once more sharded over that group; --literal: once through matrix_literal.h
  std::vector<char*> args;                              // the positional arguments
  Matrix<ZZ> rawData; std::vector<ZZ> labels; unsigned dim = 0;
  std::vector<long> thetaE; long detE = 0;
  int failures = 0;

  RegressionDriver(int argc, char* argv[], bool takesLiteral) {
    for (int i = 1; i < argc; ++i) {
      if (!strncmp(argv[i], "--devices=", 10)) { for (char* t = strtok(argv[i] + 10, ","); t; t = strtok(nullptr, ",")) devices.push_back(atoi(t)); }
      else if (takesLiteral && !strcmp(argv[i], "--literal")) literal = true;
      else args.push_back(argv[i]);
    }
  }
  long long seed(size_t at) const { return args.size() > at ? atoll(args[at]) : 1; }
  // the data file, seeded: small non-negative features and labels, as scripts/generateRandomData.py writes them; LoadData; RegressPT with exact integers
  bool load(unsigned p, unsigned dimArg, unsigned nrows, const std::string& datafile, long long seed) {
    {
      SetSeed((uint64_t)seed * 7919);
      std::ofstream out(datafile);
      out << dimArg << " " << nrows << "\n";
      for (unsigned i = 0; i < nrows; ++i) { for (unsigned j = 0; j <= dimArg; ++j) out << RandomBnd(10L) << (j == dimArg ? "\n" : " "); }
    }
    if (!LoadData(rawData, labels, dim, datafile) || dim != dimArg || rawData.NumRows() != nrows) { std::cout << "LoadData failed" << std::endl; return false; }
    std::vector<std::vector<wide>> A(dim, std::vector<wide>(dim, 0)); std::vector<wide> b(dim, 0);
    for (unsigned i = 0; i < nrows; ++i)
      for (unsigned a = 0; a < dim; ++a) { b[a] += (wide)rawData(i, a).to_long() * labels[i].to_long(); for (unsigned c = 0; c < dim; ++c) A[a][c] += (wide)rawData(i, a).to_long() * rawData(i, c).to_long(); }
    thetaE.assign(dim, 0);
    if (dim == 1) { detE = mod_p(A[0][0], p); thetaE[0] = mod_p(b[0], p); }
    else {
      detE = mod_p(det_of(A), p);
      for (unsigned i = 0; i < dim; ++i) { wide s = 0; for (unsigned k = 0; k < dim; ++k) s += cofactor(A, k, i) * b[k]; thetaE[i] = mod_p(s, p); }      // adj(i,k) = cofactor(k,i)
    }
    std::cout << "Expected values:" << std::endl;
    for (unsigned i = 0; i < dim; ++i) std::cout << "  theta[" << i << "] = " << thetaE[i] << std::endl;
    std::cout << "  Determinant: " << detE << std::endl;
    return true;
  }
  void expect(bool ok, const char* what) { std::cout << what << ": " << (ok ? "yes" : "NO") << std::endl; if (!ok) ++failures; }
  void slot0(Regression& regress, const char* what, std::vector<Ciphertext> theta, const Ciphertext& det, std::vector<std::vector<long>>* all = nullptr) {
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
  }
  // the runs on a Regression that holds the data; unmaskedCheck(plainU) is the ring's own look at every slot of the unmasked results, maskedLine
  // its wording of the count of masked slots (d = 1 has no minors to hide: Regress returns the two sums as they are).  Returns the exit code.
  template <class F> int run(Regression& regress, SeedSequence& seq, const char* maskedLine, F unmaskedCheck) {
    const FHEcontext& context = *activeContext;
    std::vector<Ciphertext> thetaU, thetaM; Ciphertext detU(context), detM(context);
    std::vector<std::vector<long>> plainU, plainM;
    regress.RegressBatched(thetaU, detU);
    slot0(regress, "batched, unmasked", thetaU, detU, &plainU);
    unmaskedCheck(plainU);
    regress.RegressBatched(thetaM, detM, seq);
    slot0(regress, "batched, masked", thetaM, detM, &plainM);
    if (dim > 1) {
      long changed = 0, slots = 0;
      for (size_t i = 0; i < plainM.size(); ++i) for (size_t j = 1; j < plainM[i].size(); ++j) { ++slots; changed += plainM[i][j] != plainU[i][j]; }
      std::cout << maskedLine << ": " << changed << " of " << slots << std::endl;
      expect(changed * 10 > slots * 9, "the masks replace the other slots");
    }
    if (!devices.empty()) {
      std::vector<Ciphertext> thetaG; Ciphertext detG(context);
      regress.RegressBatchedMultiGpu(devices, thetaG, detG, 1, &seq);
      slot0(regress, "group of ranks, masked", thetaG, detG);
    }
    if (literal) {
      std::vector<Ciphertext> thetaL; Ciphertext detL(context);
      RegressLiteral(regress, thetaL, detL);
      regress.AddNoise(thetaL, detL, seq);
      slot0(regress, "object at a time, masked", thetaL, detL);
    }
    std::cout << (failures ? "FAILED" : "OK") << std::endl;
    return failures ? 1 : 0;
  }
};
