"""The noise budget of include/fhesi_hip.h in Python integers, and a replay of the kernel's word arithmetic (fhe-si_amd/csrc/kernels_ct.hip:
round_product, round_quotient, round_residual, block_limb_max) with 64-bit wrap-around.

q = 2^logQ, z = a coefficient of toPoly(c0 + c1 t).  P = (2 p z + q) mod 2q, residual r = P - q in [-q, q), message floor((2 p z + q) / 2q) mod p.
maxres = max |r| over the coefficients, budget = max(0, logQ - bitlen(maxres))."""
import fhesi_pyref as R

M64 = (1 << 64) - 1


# ---- the definitions
def residual(z: int, logQ: int, p: int) -> int:
    q = 1 << logQ
    return (2 * p * z + q) % (2 * q) - q


def message(z: int, logQ: int, p: int) -> int:
    q = 1 << logQ
    return ((2 * p * z + q) // (2 * q)) % p


def budget_of(maxres: int, logQ: int) -> int:
    return max(0, logQ - maxres.bit_length())


def noise_of_z(zs, logQ: int, p: int):
    """-> (maxres, budget) of one ciphertext's z coefficients"""
    mx = max(abs(residual(z, logQ, p)) for z in zs)
    return mx, budget_of(mx, logQ)


def z_of(ctx: "R.Ctx", t_dcrt: dict, parts):
    """c0 + c1 t exactly as R.decrypt forms it; t_dcrt = the key's DoubleCRT (R.dcrt_from_poly(ctx, t), or rows given as {i: row})"""
    one = R.dcrt_from_poly(ctx, [1] + [0] * (ctx.phim - 1))
    cp = [R.dcrt_from_poly(ctx, part) for part in parts[:2]]
    return R.dcrt_to_poly(ctx, R.dot_product(ctx, cp, [one, t_dcrt]))


def noise(ctx: "R.Ctx", t_dcrt: dict, parts):
    """-> (message, maxres, budget) of a two-part ciphertext"""
    zs = z_of(ctx, t_dcrt, parts)
    return ([message(z, ctx.logQ, ctx.p) for z in zs],) + noise_of_z(zs, ctx.logQ, ctx.p)


def crafted_c0(r: int, logQ: int, p: int) -> int:
    """c0 of the two-part ciphertext (c0, 0) whose coefficient has the EVEN residual r in [-q, q), p odd: centred(p^-1 (r/2) mod q).
    z = c0 under any key, and 2 p c0 + q = r + q (mod 2q)."""
    assert r % 2 == 0 and p % 2 == 1 and -(1 << logQ) <= r < (1 << logQ)
    return R.reduce_logq(pow(p, -1, 1 << logQ) * (r // 2), logQ)


def boundary_residuals(logQ: int):
    """every even boundary the issue lists: -q, -q+2, -2, 0, 2, q-2, +-2^(logQ-1), and 2^j, 2^j - 2 for j at each multiple of 64 below logQ"""
    q = 1 << logQ
    out = [-q, -q + 2, -2, 0, 2, q - 2, q >> 1, -(q >> 1)]
    for j in range(64, logQ, 64):
        out += [1 << j, (1 << j) - 2]
    return [r for r in out if r % 2 == 0 and -q <= r < q]      # (logQ = 1 would make q/2 odd)


# ---- the kernel, word by word
def words_of(v: int, nw: int):
    v &= (1 << (64 * nw)) - 1
    return [(v >> (64 * i)) & M64 for i in range(nw)]


def int_of(words) -> int:
    return sum(w << (64 * i) for i, w in enumerate(words))


def kernel_coefficient(zw, logQ: int, p: int):
    """zw: nw = ceil((logQ+1)/64) two's complement words of z (what the CRT leaves).  -> (message, |r| words) as the kernel forms them."""
    nw = (logQ + 1 + 63) // 64
    assert len(zw) == nw
    top_bits = logQ + 1 - 64 * (nw - 1)
    twop = 2 * p
    P, carry = [0] * nw, 0
    for i in range(nw):                                   # round_product: 2 p zl, limb nw in carry
        xi = zw[i]
        if i == nw - 1 and top_bits < 64:
            xi &= (1 << top_bits) - 1
        lo, hi = (xi * twop) & M64, (xi * twop) >> 64
        s = (lo + carry) & M64
        carry = (hi + (s < lo)) & M64
        P[i] = s
    wq, add = logQ >> 6, 1 << (logQ & 63)                 # ... + q at word logQ >> 6, carry propagated
    for i in range(nw):
        if i >= wq:
            s = (P[i] + add) & M64
            add = int(s < add)
            P[i] = s
    carry = (carry + add) & M64
    ws, bs = (logQ + 1) >> 6, (logQ + 1) & 63             # round_quotient: the bits from logQ + 1 upward
    limb = lambda i: P[i] if i < nw else (carry if i == nw else 0)
    lo, hi = limb(ws), limb(ws + 1)
    t = ((lo >> bs) | (hi << (64 - bs))) & M64 if bs else lo
    qbit = 1 << (logQ & 63)                               # round_residual: |P mod 2q - q| from the bit test
    top_mask = ((qbit << 1) & M64) - 1 & M64
    nonneg = P[wq] & qbit
    a, borrow = [0] * nw, 0
    for i in range(nw):
        x = P[i] & top_mask if i == wq else P[i]
        qi = qbit if i == wq else 0
        d = (qi - x) & M64
        d2 = (d - borrow) & M64
        borrow = int(qi < x) | int(d < borrow)
        a[i] = ((x & ~qbit) if i == wq else x) if nonneg else d2
    return t % p, a


def limb_max(values, nw: int):
    """block_limb_max: the maximum of nw-word values by elimination from the top limb; -> its words"""
    level = [True] * len(values)
    out = [0] * nw
    for i in range(nw - 1, -1, -1):
        v = max((val[i] if lv else 0) for val, lv in zip(values, level))
        level = [lv and val[i] == v for val, lv in zip(values, level)]
        out[i] = v
    return out


def kernel_noise(zs, logQ: int, p: int, block: int = 256):
    """one ciphertext through the two launches: per-block maxima, then the lexicographic maximum of the partials per lane and the elimination.
    -> (messages, maxres words, budget)"""
    nw = (logQ + 1 + 63) // 64
    co = [kernel_coefficient(words_of(z, nw), logQ, p) for z in zs]
    parts = [limb_max([a for _, a in co[b:b + block]], nw) for b in range(0, len(co), block)]
    lanes = [[0] * nw for _ in range(64)]
    for g, v in enumerate(parts):
        if v[::-1] > lanes[g % 64][::-1]:
            lanes[g % 64] = v
    mx = limb_max(lanes, nw)
    bitlen = 0
    for i in range(nw - 1, -1, -1):
        if mx[i]:
            bitlen = 64 * i + mx[i].bit_length()
            break
    return [m for m, _ in co], mx, max(0, logQ - bitlen)
