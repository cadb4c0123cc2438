// fhesi_hoist.h -- hoisted rotations on the C++ mirror: many automorphism key switches of ONE ciphertext from one digit decomposition
// (include/fhesi_hip.h: fhesi_ksk_hoist, fhesi_ct_rotations_dev).  An extension of the mirror -- the reference rotates with
// `ctxt >>= k; keySwitch_k.ApplyKeySwitch(ctxt)` once per k (Regression.h:166-178) -- and NOT part of fhesi_host.h: include it after
// fhesi_host.h where it is wanted.  Nothing the recording evaluator instantiates calls these entries.
//
//   KeySwitchSI rot3(secretKey, 3), rot9(secretKey, 9);                 // KeySwitchSI::InitAutomorph, as before
//   HoistedKey h3 = rot3.Hoisted(3), h9 = rot9.Hoisted(9);              // derived matrices sigma_k^-1(W_k), resident in HBM
//   std::vector<Ciphertext> r = HoistedRotations(ctxt, {&h3, &h9});     // r[t] decrypts like `ctxt >>= k_t; ApplyKeySwitch`; other words
#pragma once
#include "fhesi_host.h"

namespace fhesi {

// the derived matrix of one automorphism: owns its fhesi_ksk, shared between copies
class HoistedKey {
  struct Holder {
    fhesi_ksk* k;
    explicit Holder(fhesi_ksk* kk) : k(kk) {}
    ~Holder() { if (k) fhesi_ksk_free(k); }
    Holder(const Holder&) = delete;
    Holder& operator=(const Holder&) = delete;
  };
  std::shared_ptr<Holder> h;
  const FHEcontext* context;
  unsigned k_;
 public:
  HoistedKey(const FHEcontext& c, fhesi_ksk* derived, unsigned k) : h(std::make_shared<Holder>(derived)), context(&c), k_(k) {}
  const fhesi_ksk* handle() const { return h->k; }
  unsigned k() const { return k_; }
  const FHEcontext& GetContext() const { return *context; }
  size_t bytes() const { return fhesi_ksk_bytes(h->k); }       // the rows; the auxiliary table comes on top at the first use
};

// this matrix -- made by KeySwitchSI(secretKey, k) -- moved by sigma_k^-1: the operand of HoistedRotations for the same k
inline HoistedKey KeySwitchSI::Hoisted(unsigned k) const {
  fhesi_ksk* out = nullptr;
  ck(fhesi_ksk_hoist(device_key(), (int64_t)k, &out));
  return HoistedKey(context, out, k);
}

// out[t] = the rotation of c by keys[t]->k(); a null entry is the identity (the reduced copy: diagonal 0 of a matrix-vector product).
// One device call: the digits of c are decomposed and transformed once for all keys.
inline std::vector<Ciphertext> HoistedRotations(const Ciphertext& c, const std::vector<const HoistedKey*>& keys) {
  Ciphertext in(c);
  if (in.isScaledUp() || in.size() != 2) Error("HoistedRotations: expects an unscaled 2-part ciphertext");
  const FHEcontext* context = nullptr;
  for (const HoistedKey* k : keys) if (k) { if (context && context != &k->GetContext()) Error("Incompatible contexts."); context = &k->GetContext(); }
  std::vector<Ciphertext> out;
  if (keys.empty()) return out;
  if (!context) { out.assign(keys.size(), c); return out; }
  fhesi_ctx* h = context->handle();
  const long n = context->zMstar.phiM(); const int nl = (int)((context->logQ + 63) / 64);
  const size_t words = (size_t)2 * n * nl, T = keys.size();
  std::vector<uint64_t> host(words, 0), res(T * words);
  for (int part = 0; part < 2; ++part) poly_to_limbs(in[(unsigned)part].poly /* (a recorded value is evaluated here) */, &host[((size_t)part * n) * nl], n, nl);
  std::vector<const fhesi_ksk*> hs; std::vector<int64_t> ks;
  for (const HoistedKey* k : keys) { hs.push_back(k ? k->handle() : nullptr); ks.push_back(k ? (int64_t)k->k() : 1); }
  void *d_in, *d_out;
  ck(fhesi_dev_alloc(h, words * 8, &d_in));
  int rc = fhesi_dev_alloc(h, T * words * 8, &d_out);
  if (rc) { fhesi_dev_free(h, d_in); ck(rc); }
  rc = fhesi_dev_upload(h, d_in, host.data(), words * 8);
  if (!rc) rc = fhesi_ct_rotations_dev(h, hs.data(), ks.data(), (int32_t)T, (int32_t)context->logQ, (int32_t)context->decompSize, (const uint64_t*)d_in, nl, 1, (uint64_t*)d_out, nl);
  if (!rc) rc = fhesi_dev_download(h, res.data(), d_out, res.size() * 8);
  fhesi_dev_free(h, d_in); fhesi_dev_free(h, d_out);
  ck(rc);
  out.assign(T, Ciphertext(*context));
  for (size_t t = 0; t < T; ++t) {
    out[t].Initialize(2, *context);
    for (int part = 0; part < 2; ++part) limbs_to_poly(out[t][(unsigned)part].poly, &res[t * words + ((size_t)part * n) * nl], n, nl);
  }
  return out;
}

}  // namespace fhesi
