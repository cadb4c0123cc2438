// test_regression_data.cpp -- the reference's Test_Regression driver end to end (Test_Regression.cpp:10-67), with NUMBERS in and NUMBERS out:
//
//   test_regression_data p generator dim nrows datafile [seed] [--devices=0,0] [--literal]
//
// writes a seeded data file in the reference's format, then runs
//   LoadData -> BatchData -> AddDataSlots -> RegressBatched (masked with GenerateNoise) -> DecryptSlotsBatch -> slot 0
// and compares slot 0 of theta[i] and det with the integer regression taken modulo p (regression_driver.h, which holds everything this program
// shares with test_regression_pow2.cpp).  Context as in Test_Regression.cpp:85-125: m = p - 1, logQ from the same formula.
// --devices runs the waves once more sharded over that group (a repeated GPU gives a loopback group); --literal once through the
// object-at-a-time evaluator (matrix_literal.h).  Exit code 0 on success.
#include "regression_driver.h"

int main(int argc, char* argv[]) {
  RegressionDriver D(argc, argv, true);
  if (D.args.size() < 5) { std::cout << "usage: test_regression_data p generator dim nrows datafile [seed] [--devices=0,0] [--literal]" << std::endl; return 1; }
  const unsigned p = atoi(D.args[0]), g = atoi(D.args[1]), nrows = atoi(D.args[3]);
  const long long seed = D.seed(5);
  if (!D.load(p, atoi(D.args[2]), nrows, D.args[4], seed)) return 1;
  const unsigned dim = D.dim;
  const Matrix<ZZ>& rawData = D.rawData; const std::vector<ZZ>& labels = D.labels;

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
    D.expect(ok, "BatchData plaintexts decode to the data");
    // Plaintext >>= 1 moves slot j + 1 into slot j; += and == act on the message
    Plaintext a = ptxtData[0][0], r = a; r >>= 1;
    std::vector<long> sa, sr; a.DecodeSlots(sa, false); r.DecodeSlots(sr, false);
    bool rot = true; for (size_t j = 0; j < sa.size(); ++j) rot = rot && sr[j] == sa[(j + 1) % sa.size()];
    Plaintext sum = a; sum += r; sum -= r;
    D.expect(rot && sum == a && !(r == a), "Plaintext >>= 1 rotates left by one, += / -= / == hold");
  }

  SetSeed((uint64_t)seed);
  Regression regress(context);
  SeedSequence seq((uint64_t)seed * 0x9e3779b97f4a7c15ull + 1, (uint64_t)seed * 0xbf58476d1ce4e5b9ull + 2);
  regress.AddDataSlots(rawData, labels, seq);
  return D.run(regress, seq, "masked slots that differ from the unmasked partial sums", [](const std::vector<std::vector<long>>&) {});
}
