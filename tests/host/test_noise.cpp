// test_noise.cpp -- TEST HARNESS for FHESISecKey::NoiseBudget / NoiseBudgetBatch (fhe-si_amd/host/fhesi_keys.h): the budget of a ciphertext that
// lives in HBM (recording on: one device call on it), of the same ciphertext uploaded for the call (recording off) and from toPoly in ZZ
// (NoiseBudgetObjects, which touches no noise kernel) must be one number -- on fresh encryptions, after a multiplication and key switch, and on
// a recorded product that nobody has looked at before the call.
//
//   test_noise [m logQ p g [seed]]      exit code = number of failed checks
#include <iostream>

#include "../../fhe-si_amd/host/fhesi_serialization.h"

using namespace fhesi;
namespace fhesi { FHEcontext* activeContext = nullptr; }

static int failures = 0;
static void expect(bool ok, const char* what) { std::cout << (ok ? "  ok   " : "  FAIL ") << what << std::endl; if (!ok) ++failures; }
static Ciphertext host_copy(const Ciphertext& c) { Ciphertext r = c; r.parts.host(); return r; }
struct Eager { bool was; Eager() : was(LazyCiphertexts()) { LazyCiphertexts() = false; } ~Eager() { LazyCiphertexts() = was; } };   // statements run at once inside the scope

int main(int argc, char* argv[]) {
  const unsigned m = argc >= 5 ? atoi(argv[1]) : 64, logQ = argc >= 5 ? atoi(argv[2]) : 100, p = argc >= 5 ? atoi(argv[3]) : 257, g = argc >= 5 ? atoi(argv[4]) : 3;
  SetSeed((uint64_t)(argc >= 6 ? atoll(argv[5]) : 1));
  FHEcontext context(m, logQ, p, g);
  activeContext = &context;
  context.SetUpSIContext();
  FHESISecKey secretKey(context);
  FHESIPubKey publicKey(secretKey);
  KeySwitchSI keySwitch(secretKey);
  const long n = context.zMstar.phiM(), count = 4;
  if (!LazyCiphertexts()) { std::cout << "recording is off (FHESI_EAGER): this program compares the recorded form with it, nothing to do" << std::endl << "OK" << std::endl; return 0; }
  std::cout << "m=" << m << " phi(m)=" << n << " logQ=" << logQ << " p=" << p << " primes=" << context.numPrimes() << std::endl;
  std::vector<Plaintext> pts(count);
  for (auto& x : pts) { x.message.resize(n); for (auto& c : x.message) c = RandomBnd((long)p); }
  std::vector<Ciphertext> cts;
  publicKey.EncryptBatchSeeded(cts, pts, 21, 0);

  // the three statements of the budget on one vector of ciphertexts
  auto three_ways = [&](std::vector<Ciphertext>& v, const char* what) {
    std::vector<long> recorded, batch, at_once, objects;
    for (auto& c : v) recorded.push_back(secretKey.NoiseBudget(c));
    secretKey.NoiseBudgetBatch(batch, v);
    std::vector<Ciphertext> host; for (auto& c : v) host.push_back(host_copy(c));
    { Eager e; secretKey.NoiseBudgetBatch(at_once, host); for (auto& c : host) objects.push_back(secretKey.NoiseBudget(c)); }
    std::cout << what << ": budgets"; for (long b : recorded) std::cout << " " << b; std::cout << std::endl;
    expect(recorded == batch, "NoiseBudget equals NoiseBudgetBatch with recording on");
    expect(recorded == at_once, "... equals NoiseBudgetBatch with recording off");
    expect(recorded == objects, "... equals the budget from toPoly in ZZ");
    return recorded;
  };
  std::vector<long> fresh = three_ways(cts, "fresh");
  bool positive = true; for (long b : fresh) positive = positive && b > 0 && b < (long)logQ;
  expect(positive, "fresh encryptions have a positive budget below logQ");

  // after one multiplication and key switch; the product of cts[0] and cts[1] is recorded and NOT looked at before NoiseBudget forces it
  Ciphertext pending = cts[0]; pending *= cts[1]; keySwitch.ApplyKeySwitch(pending);
  const long b_pending = secretKey.NoiseBudget(pending);
  std::vector<Ciphertext> prods;
  for (long c = 0; c < count; ++c) { Ciphertext t = cts[c]; t *= cts[(c + 1) % count]; keySwitch.ApplyKeySwitch(t); prods.push_back(t); }
  std::vector<long> after = three_ways(prods, "after one multiplication");
  expect(b_pending == after[0], "a recorded product that was not looked at before the call has the budget of the same product evaluated");
  bool dropped = true; for (long c = 0; c < count; ++c) dropped = dropped && after[c] <= fresh[c] && after[c] <= fresh[(c + 1) % count];
  expect(dropped, "the budget does not rise across a multiplication");
  bool right = true;
  for (long c = 0; c < count; ++c) if (after[c] > 0) {
    Plaintext got; secretKey.Decrypt(got, prods[c]);
    Eager e; Ciphertext a = host_copy(cts[c]), b = host_copy(cts[(c + 1) % count]); a *= b; keySwitch.ApplyKeySwitch(a);
    Plaintext want; secretKey.Decrypt(want, a);
    right = right && got.message == want.message && secretKey.NoiseBudget(a) == after[c];
  }
  expect(right, "products with a positive budget decrypt alike recorded and at once, with one budget");
  std::cout << (failures ? "FAILED" : "OK") << std::endl;
  return failures;
}
