// test_regression_pow2.cpp -- the data-file regression driver of test_regression_data.cpp on a POWER-OF-TWO ring, where the slots form two rows
// (m = 2^k, p = 1 mod m; include/fhesi_hip.h, "the TWO-ROW space"):
//
//   test_regression_pow2 m p generator dim nrows datafile [seed] [--devices=0,0]        dim = 1 or 2
//
// writes a seeded data file, then runs
//   LoadData -> BatchData -> AddDataSlots -> RegressBatched (unmasked, and masked with GenerateNoise) -> DecryptSlotsBatch
// and compares slot 0 of theta[i] and det with the integer regression modulo p (regression_driver.h).  On the way it checks what is
// particular to these rings: Rows() / Cols(), Plaintext >>= rotating each row, SwapRows, the exponent list g, g^2, ..., g^(n/4), m - 1 of
// Regression, and that the unmasked results carry the total in EVERY slot.  m / 2 slots per ciphertext, all usable.  Exit code 0 on success.
#include "regression_driver.h"

int main(int argc, char* argv[]) {
  RegressionDriver D(argc, argv, false);
  if (D.args.size() < 6) { std::cout << "usage: test_regression_pow2 m p generator dim nrows datafile [seed] [--devices=0,0]" << std::endl; return 1; }
  const unsigned m = atoi(D.args[0]), p = atoi(D.args[1]), g = atoi(D.args[2]), dimArg = atoi(D.args[3]), nrows = atoi(D.args[4]);
  const long long seed = D.seed(6);
  if (dimArg < 1 || dimArg > 2) { std::cout << "dim must be 1 or 2" << std::endl; return 1; }
  if (!D.load(p, dimArg, nrows, D.args[5], seed)) return 1;
  const unsigned dim = D.dim;
  const Matrix<ZZ>& rawData = D.rawData; const std::vector<ZZ>& labels = D.labels;

  // one multiplication level per dimension on top of the inner products; p and the m / 2 slots both enter the noise of a level
  const unsigned nSlots = m / 2, nBlocks = (nrows + nSlots - 1) / nSlots, xi = std::max(nBlocks, dim), logQ = 100 + 100 * dim;
  FHEcontext context(m, logQ, p, g, 3);
  activeContext = &context;
  context.SetUpSIContext(xi);
  const PlaintextSpace& space = context.GetPlaintextSpace();
  std::cout << "regression on data: p=" << p << " m=" << m << " slots=" << space.GetTotalSlots() << " usable=" << space.GetUsableSlots() << " rows=" << space.Rows()
            << " cols=" << space.Cols() << " logQ=" << logQ << " dim=" << dim << " data rows=" << nrows << " blocks=" << nBlocks << std::endl;
  D.expect(space.Rows() == 2 && space.Cols() == m / 4 && space.GetTotalSlots() == nSlots && space.GetUsableSlots() == nSlots, "two rows of m / 4 columns, every slot usable");

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
    D.expect(ok, "BatchData plaintexts decode to the data");
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
    D.expect(rot && sum == a && !(r == a), "Plaintext >>= 3 rotates both rows left by three, += / -= / == hold");
    D.expect(swp && c == s, "SwapRows exchanges the rows and equals X -> X^(m-1) on the coefficients");
  }

  SetSeed((uint64_t)seed);
  Regression regress(context);
  {
    const std::vector<unsigned>& ks = regress.AutomorphismExponents();
    unsigned lg = 0; while ((1u << lg) < nSlots) ++lg;
    bool ok = ks.size() == lg && ks.back() == m - 1 && ks[0] == g % m;
    for (size_t i = 0; ok && i + 1 < ks.size(); ++i) ok = ks[i] != 1 && (i == 0 || ks[i] == (unsigned)(((unsigned long)ks[i - 1] * ks[i - 1]) % m));
    D.expect(ok, "the exponents of the total sum are g, g^2, g^4, ..., then m - 1");
  }
  SeedSequence seq((uint64_t)seed * 0x9e3779b97f4a7c15ull + 1, (uint64_t)seed * 0xbf58476d1ce4e5b9ull + 2);
  regress.AddDataSlots(rawData, labels, seq);
  return D.run(regress, seq, "masked slots that differ from the unmasked ones", [&](const std::vector<std::vector<long>>& plainU) {
    bool same = true;
    for (auto& v : plainU) { same = same && v.size() == nSlots; for (long x : v) same = same && x == v[0]; }
    D.expect(same, "unmasked: the total reaches every slot of both rows");
  });
}
