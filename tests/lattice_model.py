"""Strided and dilated convolutions and sum pooling on packed slots in slot terms (numpy / Python ints): the model of fhesi_conv2d_lattice_*,
fhesi_pool2d_plan, fhesi_ct_pool2d_dev and fhesi_slots_lattice_columns, built on conv_model.

The plane H x W of conv_model is never compacted.  It carries a lattice step (sy, sx), sy | H, sx | W: logical pixel (a, b) of the Hl x Wl = H/sy x W/sx
logical plane sits at physical pixel (a sy, b sx); slots off the lattice are don't care on input.  Stride (ty, tx), ty | Hl, tx | Wl; dilation (ey, ex);
the output step is (sy ty, sx tx).

    definition  out[I](a', b') = b[I] + sum_J sum_dy sum_dx K[I][J][dy][dx] in[J](a' ty + (dy - ah) ey, b' tx + (dx - aw) ex),  logical pixels outside
                Hl x Wl = 0; EVERY output slot off the output lattice is exactly 0, bias included
    offsets     t = dy kw + dx, u = (dy - ah) ey sy, v = (dx - aw) ex sx (physical pixels), a_t = (u W + v) mod cols,
                mu_t[i] = [sy ty | y and sx tx | x and 0 <= y + u < H and 0 <= x + v < W]
    flat, split as in conv_model, the split form's plaintexts moved back by the giant amount (u W) mod cols; the bias under the output lattice's factor

    sum pooling  non-overlapping windows of kh x kw logical pixels, kh sy | H and kw sx | W: no mask, no plaintext product,
                 out = sum_{dy < kh} rot_{(dy sy W) mod cols}( sum_{dx < kw} rot_{(dx sx) mod cols}(in) ),  output step (sy kh, sx kw)
                 form 1: per direction the k - 1 rotations of ONE value, summed with it; form 2 (kw, kh powers of two): doubling folds

A plain module, imported like conv_model."""
import numpy as np

import bsgs_model as BM
import conv_model as CM

FLAT, SPLIT = CM.FLAT, CM.SPLIT
HOISTED, DOUBLING = 1, 2
TRIVIAL = ((1, 1), (1, 1), (1, 1))
CLAMP = 1 << 62


def clamp(a):
    return max(-CLAMP, min(CLAMP, a))


def offsets(kh, kw, ah, aw, step, dilation):
    """(u, v) of entry t = dy kw + dx in physical pixels (clamped into +-2^62, as the header's products are)"""
    return [(clamp(clamp((dy - ah) * dilation[0]) * step[0]), clamp(clamp((dx - aw) * dilation[1]) * step[1])) for dy in range(kh) for dx in range(kw)]


def refused(cols, H, W, Cin, Cout, kh, kw, ah, aw, step, stride, dilation, form=0):
    """None, or the word of the condition the shape breaks (the order fhesi_conv2d_lattice_plan checks them in)"""
    if cols < 1 or cols > 1 << 20:
        return "outside [1, 2^20]"
    if min(H, W, Cin, Cout, kh, kw) < 1:
        return "every size at least 1"
    if H * W > cols or cols % (H * W):
        return "does not divide the row"
    if min(step + stride + dilation) < 1:
        return "every factor at least 1"
    if H % step[0] or W % step[1]:
        return f"the step ({step[0]}, {step[1]}) does not divide the {H} x {W} plane"
    if (H // step[0]) % stride[0] or (W // step[1]) % stride[1]:
        return f"the stride ({stride[0]}, {stride[1]}) does not divide the logical plane of {H // step[0]} x {W // step[1]} pixels"
    if not (0 <= ah < kh and 0 <= aw < kw):
        return "anchor"
    for dy in range(kh):
        for dx in range(kw):
            u, v = clamp(clamp((dy - ah) * dilation[0]) * step[0]), clamp(clamp((dx - aw) * dilation[1]) * step[1])
            if abs(u) >= H or abs(v) >= W:
                return f"the offset ({u}, {v}) has an empty mask"
    if Cout * Cin * kh * kw > 65535:
        return "per handle"
    if form not in (0, FLAT, SPLIT):
        return "form"
    return None


def plan(cols, H, W, Cin, Cout, kh, kw, ah, aw, step, stride, dilation, form=0):
    """conv_model.plan with the amounts of the stretched offsets, and the output step"""
    assert refused(cols, H, W, Cin, Cout, kh, kw, ah, aw, step, stride, dilation, form) is None
    if not form:
        form = SPLIT if CM.key_switches(Cin, Cout, kh, kw, SPLIT) < CM.key_switches(Cin, Cout, kh, kw, FLAT) else FLAT
    off = offsets(kh, kw, ah, aw, step, dilation)
    if form == FLAT:
        amounts = [(u * W + v) % cols for u, v in off]
        terms = Cin * kh * kw
    else:
        amounts = [off[dx][1] % cols for dx in range(kw)] + [(off[dy * kw][0] * W) % cols for dy in range(kh)]
        terms = Cin * kw
    return {"form": form, "nh": len(amounts), "key_switches": CM.key_switches(Cin, Cout, kh, kw, form), "terms": terms, "amounts": amounts,
            "out_step": (step[0] * stride[0], step[1] * stride[1])}


def lattice(H, W, step, rows, cols):
    """[sy | y and sx | x] on every row"""
    i = np.arange(cols) % (H * W)
    y, x = i // W, i % W
    return np.tile(((y % step[0] == 0) & (x % step[1] == 0)).astype(np.int64), rows)


def direct(K, bias, xs, H, W, anchor, step, stride, dilation, p, rows):
    """the definition on slot values xs [Cin][rows * cols] -> [Cout][rows * cols] modulo p: the logical planes read off the lattice, convolved, strided,
    and written onto the output lattice of an all-zero plane"""
    K = np.asarray(K, dtype=object)
    Cout, Cin, kh, kw = K.shape
    ah, aw = anchor
    (sy, sx), (ty, tx), (ey, ex) = step, stride, dilation
    img = np.asarray(CM.images(np.asarray(xs, dtype=object), H, W, rows), dtype=object)      # [Cin][rows][nimg][H][W]
    log = img[..., ::sy, ::sx]                                                               # [Cin][rows][nimg][Hl][Wl]
    Hl, Wl = H // sy, W // sx
    out = np.zeros((Cout,) + img.shape[1:], dtype=object)
    for I in range(Cout):
        for a in range(Hl // ty):
            for b in range(Wl // tx):
                acc = np.zeros(img.shape[1:3], dtype=object) + (0 if bias is None else int(bias[I]))
                for J in range(Cin):
                    for dy in range(kh):
                        for dx in range(kw):
                            yy, xx = a * ty + (dy - ah) * ey, b * tx + (dx - aw) * ex
                            if 0 <= yy < Hl and 0 <= xx < Wl:
                                acc = acc + int(K[I][J][dy][dx]) * log[J, :, :, yy, xx]
                out[I, :, :, a * ty * sy, b * tx * sx] = acc % p
    return out.reshape(Cout, -1)


def mask(u, v, H, W, out_step, rows, cols):
    """mu_t on every row: the output lattice's factor and the range tests of the physical offset (u, v)"""
    i = np.arange(cols) % (H * W)
    y, x = i // W, i % W
    on = (y % out_step[0] == 0) & (x % out_step[1] == 0) & (y + u >= 0) & (y + u < H) & (x + v >= 0) & (x + v < W)
    return np.tile(on.astype(np.int64), rows)


def prepared(K, H, W, anchor, step, stride, dilation, rows, cols, form):
    """[Cout][Cin][kh kw][rows * cols]: w^{IJ}_t (flat) or w'^{IJ}_t (split), entries as they are in K"""
    K = np.asarray(K, dtype=object)
    Cout, Cin, kh, kw = K.shape
    out_step = (step[0] * stride[0], step[1] * stride[1])
    out = np.zeros((Cout, Cin, kh * kw, rows * cols), dtype=object)
    for t, (u, v) in enumerate(offsets(kh, kw, anchor[0], anchor[1], step, dilation)):
        mu = np.asarray(mask(u, v, H, W, out_step, rows, cols), dtype=object)
        if form == SPLIT:
            mu = BM.rotate_values(mu, -((u * W) % cols), rows)
        for I in range(Cout):
            for J in range(Cin):
                out[I][J][t] = int(K[I][J][t // kw][t % kw]) * mu
    return out


def bias_values(bias, H, W, out_step, p, rows, cols):
    """[Cout][rows * cols]: b[I] modulo p on the output lattice, 0 off it"""
    on = np.asarray(lattice(H, W, out_step, rows, cols), dtype=object)
    return np.stack([(int(b) % p) * on for b in bias])


def schedule(K, bias, xs, H, W, anchor, step, stride, dilation, p, rows, form, counts=None):
    """the schedule of the run call on slot values xs [Cin][rows * cols] -> [Cout][rows * cols] modulo p; counts: a dict that receives the rotations the
    schedule itself runs on values that stand for ciphertexts (the identity not counted)"""
    K = np.asarray(K, dtype=object)
    Cout, Cin, kh, kw = K.shape
    cols = len(xs[0]) // rows
    pl = plan(cols, H, W, Cin, Cout, kh, kw, anchor[0], anchor[1], step, stride, dilation, form)
    w = prepared(K, H, W, anchor, step, stride, dilation, rows, cols, pl["form"]) % p
    B, G = (kh * kw, 1) if pl["form"] == FLAT else (kw, kh)
    kb, kg = pl["amounts"][:B], ([0] if pl["form"] == FLAT else pl["amounts"][B:])
    ran = 0
    babies = [[np.asarray(BM.rotate_values(xs[J], a, rows), dtype=object) for a in kb] for J in range(Cin)]      # once per input channel
    ran += Cin * sum(1 for a in kb if a)
    out = []
    for I in range(Cout):
        acc = np.zeros(rows * cols, dtype=object)
        for g in range(G):
            inner = np.zeros(rows * cols, dtype=object)
            for J in range(Cin):
                for j in range(B):
                    inner = (inner + w[I][J][g * B + j] * babies[J][j]) % p
            acc = (acc + BM.rotate_values(inner, kg[g], rows)) % p                                                  # once per output channel
            ran += 1 if kg[g] else 0
        if bias is not None:
            acc = (acc + bias_values([bias[I]], H, W, pl["out_step"], p, rows, cols)[0]) % p
        out.append(acc)
    if counts is not None:
        counts["key_switches"] = ran
    return np.stack(out)


# ------------------------------------------------------------------------------------------------ sum pooling
def is_pow2(k):
    return k >= 1 and not k & (k - 1)


def pool_refused(cols, H, W, kh, kw, sy, sx, form=0):
    """None, or the word of the condition the shape breaks (the order fhesi_pool2d_plan checks them in)"""
    if cols < 1 or cols > 1 << 20:
        return "outside [1, 2^20]"
    if min(H, W, kh, kw, sy, sx) < 1:
        return "every size at least 1"
    if H * W > cols or cols % (H * W):
        return "does not divide the row"
    if H % sy or W % sx:
        return f"the step ({sy}, {sx}) does not divide the {H} x {W} plane"
    if kh > H // sy or kw > W // sx or (H // sy) % kh or (W // sx) % kw:
        return f"windows of {kh} x {kw} pixels do not tile the logical plane of {H // sy} x {W // sx} pixels"
    if form not in (0, HOISTED, DOUBLING):
        return "form"
    if form == DOUBLING and not (is_pow2(kh) and is_pow2(kw)):
        return "form 2 (doubling) takes windows of powers of two"
    return None


def pool_key_switches(kh, kw, form):
    return (kw - 1) + (kh - 1) if form == HOISTED else (kw.bit_length() - 1) + (kh.bit_length() - 1)


def pool_plan(cols, H, W, kh, kw, sy, sx, form=0):
    """form 0: the form of fewer key switches, form 1 on a tie (fewer levels).  amounts: the horizontal ones, then the vertical ones"""
    assert pool_refused(cols, H, W, kh, kw, sy, sx, form) is None
    if not form:
        form = DOUBLING if is_pow2(kh) and is_pow2(kw) and pool_key_switches(kh, kw, DOUBLING) < pool_key_switches(kh, kw, HOISTED) else HOISTED
    if form == HOISTED:
        hor, ver = [(dx * sx) % cols for dx in range(1, kw)], [(dy * sy * W) % cols for dy in range(1, kh)]
        levels = (kw > 1) + (kh > 1)
    else:
        hor = [((1 << j) * sx) % cols for j in range(kw.bit_length() - 1)]
        ver = [((1 << j) * sy * W) % cols for j in range(kh.bit_length() - 1)]
        levels = len(hor) + len(ver)
    return {"form": form, "nh": len(hor) + len(ver), "nhor": len(hor), "key_switches": pool_key_switches(kh, kw, form), "levels": levels,
            "amounts": hor + ver, "out_step": (sy * kh, sx * kw)}


def pool_formula(x, H, W, kh, kw, sy, sx, p, rows):
    """the defining formula on slot values x [rows * cols] modulo p: every slot, the cyclic sums off the output lattice included"""
    x = np.asarray(x, dtype=object)
    cols = len(x) // rows
    inner = np.zeros(len(x), dtype=object)
    for dx in range(kw):
        inner = (inner + BM.rotate_values(x, (dx * sx) % cols, rows)) % p
    out = np.zeros(len(x), dtype=object)
    for dy in range(kh):
        out = (out + BM.rotate_values(inner, (dy * sy * W) % cols, rows)) % p
    return out


def pool_direct(x, H, W, kh, kw, sy, sx, p, rows):
    """the window sums of the logical planes, read off the lattice: [rows][nimg][Hl / kh][Wl / kw] modulo p -- what the slots ON the output lattice hold"""
    img = np.asarray(CM.images(np.asarray(x, dtype=object), H, W, rows), dtype=object)[..., ::sy, ::sx]      # [rows][nimg][Hl][Wl]
    Hl, Wl = H // sy, W // sx
    return img.reshape(img.shape[:2] + (Hl // kh, kh, Wl // kw, kw)).sum(axis=(3, 5)) % p


def pool_schedule(x, H, W, kh, kw, sy, sx, p, rows, form, counts=None):
    """the schedule of fhesi_ct_pool2d_dev on slot values x [rows * cols] modulo p"""
    y = np.asarray(x, dtype=object) % p
    cols = len(y) // rows
    pl = pool_plan(cols, H, W, kh, kw, sy, sx, form)
    ran = levels = 0
    if pl["form"] == HOISTED:
        for amounts in (pl["amounts"][:pl["nhor"]], pl["amounts"][pl["nhor"]:]):
            if amounts:
                y = (y + sum(np.asarray(BM.rotate_values(y, a, rows), dtype=object) for a in amounts)) % p      # every rotation of ONE value
                ran, levels = ran + len(amounts), levels + 1
    else:
        for a in pl["amounts"]:
            y = (y + BM.rotate_values(y, a, rows)) % p
            ran, levels = ran + 1, levels + 1
    if counts is not None:
        counts["key_switches"], counts["levels"] = ran, levels
    return y


# ------------------------------------------------------------------------------------------------ the bridge to a dense layer
def lattice_columns(M, nch, H, W, step):
    """M [R][nch Hl Wl] over logical pixels -> M' [R][nch P] over the slots of the planes: column c P + (a sy) W + b sx takes column c Hl Wl + a Wl + b,
    the columns off the lattice are zero"""
    M = np.asarray(M)
    sy, sx = step
    Hl, Wl = H // sy, W // sx
    assert M.ndim == 2 and M.shape[1] == nch * Hl * Wl
    out = np.zeros((M.shape[0], nch, H, W), dtype=M.dtype)
    out[:, :, ::sy, ::sx] = M.reshape(M.shape[0], nch, Hl, Wl)
    return out.reshape(M.shape[0], nch * H * W)
