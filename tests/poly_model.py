"""The model of the polynomial evaluation on packed slots (fhesi_ct_poly_eval_dev; fhe-si_amd/csrc/poly_plan.h): the Paterson-Stockmeyer plan and the
schedule of products and scalar combinations, over Python integers.  The normative statement of both: the header and the library follow this file.
A plain module, imported like slots_model.

y = f(x) = sum_{k <= d} c_k x^k slot by slot, with B baby powers x^1 .. x^B and the giants x^(gB), g = 2 .. G - 1, G = floor(d / B) + 1:
  f(x) = sum_{g < G} u_g(x) x^(gB),   u_g(x) = sum_{j < B, gB + j <= d} c_(gB+j) x^j.
Every power is a product of two earlier powers (halving: depth ceil(log2)); an inner sum u_g is a scalar linear combination of the babies with its
constant; the outer sum over g >= 1 is ONE sum of products with one key switch; group 0, the groups that are a constant alone and that sum close in
one more scalar linear combination.

A schedule names ciphertexts by references: ("x", k) the power x^k, ("u", g) an inner sum, ("W",) the outer sum."""


def clog2(v):
    """ceil(log2(v)) for v >= 1"""
    return (v - 1).bit_length()


MAX_DEGREE = 4096


def counts(d, B):
    """the plan of a DENSE polynomial of degree d with B baby powers: every coefficient counted non-zero"""
    if not 1 <= d <= MAX_DEGREE:
        raise ValueError(f"degree {d} outside 1 .. {MAX_DEGREE}")
    if not 1 <= B <= d:
        raise ValueError(f"{B} baby powers outside 1 .. {d}")
    G = d // B + 1
    npairs = sum(1 for g in range(1, G) if B >= 2 and g * B + 1 <= d)       # the groups g >= 1 that hold a term x^j, j >= 1
    powers = (B - 1) + max(G - 2, 0)
    return {"B": B, "G": G, "nprod": powers + npairs, "nks": powers + (1 if npairs else 0), "depth": clog2(B) + clog2(max(G - 1, 1)) + (1 if npairs else 0)}


def plan(d, baby=0):
    """baby = 0: the B of least key switches; of equal key switches the smaller depth; of equal depth the larger B"""
    if baby:
        return counts(d, baby)
    if not 1 <= d <= MAX_DEGREE:
        raise ValueError(f"degree {d} outside 1 .. {MAX_DEGREE}")
    return min((counts(d, B) for B in range(1, d + 1)), key=lambda c: (c["nks"], c["depth"], -c["B"]))


def residues(c, p):
    """(c mod p in [0, p), its centred representative in (-p/2, p/2])"""
    r = c % p
    return r, (r if 2 * r <= p else r - p)


def pool_entry(k, B):
    """where the power x^k lives in the pool of one item: the babies x^1 .. x^B at 0 .. B - 1, the giants x^(gB), g >= 2, at B + g - 2"""
    if 1 <= k <= B:
        return k - 1
    assert k % B == 0 and k // B >= 2
    return B + k // B - 2


def schedule(coef, p, baby=0):
    """coef[0 .. d] any integers, p >= 2 -> the schedule:
      B, G;
      levels: [[(k, ka, kb)]]   x^k = MulRelin(x^ka, x^kb); one list per call of the sum-of-products wave, every item's products in it
      inner:  [(g, [(c, j)], konst)]   u_g = LinComb(c x^j ...; konst), ascending g and j; ALL of them one call of the scalar combination
      pairs:  [(g, gB)]   W = KeySwitch(sum u_g x^(gB)), ascending g: one group per item, one key switch (absent: no W)
      final:  ([(c, ref)], konst)   y = LinComb(...; konst): group 0's terms in ascending j, the constant-only groups in ascending g, then (1, W)"""
    d = len(coef) - 1
    B = plan(d, baby)["B"]
    G = d // B + 1
    cbar, chat = zip(*(residues(int(c), p) for c in coef))
    levels = []
    for lv in range(1, clog2(B) + 1):                                       # babies of level ceil(log2 j)
        levels.append([(j, (j + 1) // 2, j // 2) for j in range((1 << (lv - 1)) + 1, min(1 << lv, B) + 1)])
    for lv in range(1, clog2(max(G - 1, 1)) + 1):                           # giants of level ceil(log2 g)
        levels.append([(g * B, (g + 1) // 2 * B, g // 2 * B) for g in range((1 << (lv - 1)) + 1, min(1 << lv, G - 1) + 1)])
    inner, pairs, final = [], [], []
    for g in range(G):
        terms = [(chat[g * B + j], j) for j in range(1, B) if g * B + j <= d and chat[g * B + j]]
        if g == 0:
            final += [(c, ("x", j)) for c, j in terms]
        elif terms:
            inner.append((g, terms, cbar[g * B]))
            pairs.append((g, g * B))
    final += [(chat[g * B], ("x", g * B)) for g in range(1, G) if g not in {q[0] for q in pairs} and chat[g * B]]
    if pairs:
        final.append((1, ("W",)))
    return {"B": B, "G": G, "levels": levels, "inner": inner, "pairs": pairs, "final": (final, cbar[0])}


def evaluate(s, v, p):
    """the schedule on the integer v modulo p: what every slot of the result holds"""
    x = {1: v % p}
    for level in s["levels"]:
        new = {k: x[a] * x[b] % p for k, a, b in level}                     # (a level reads earlier levels only)
        assert not set(new) & set(x)
        x.update(new)
    u = {g: (sum(c * x[j] for c, j in terms) + konst) % p for g, terms, konst in s["inner"]}
    W = sum(u[g] * x[k] for g, k in s["pairs"]) % p
    terms, konst = s["final"]
    return (sum(c * (W if ref[0] == "W" else x[ref[1]]) for c, ref in terms) + konst) % p


def key_switches(s):
    return sum(len(level) for level in s["levels"]) + (1 if s["pairs"] else 0)


def horner(coef, v, p):
    y = 0
    for c in reversed(coef):
        y = (y * v + c) % p
    return y
