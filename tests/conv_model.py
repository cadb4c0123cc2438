"""Convolution layers on packed slots in slot terms (numpy / Python ints): the model of fhesi_conv2d_* and fhesi_ct_conv2d_dev, built on bsgs_model.

The space has `rows` rows of `cols` slots; a rotation by a moves every row a slots to the left.  An H x W plane, P = H W | cols: slot (r, i) holds pixel
(y, x) = ((i mod P) div W, (i mod P) mod W) of image (r, i div P).  One channel per plaintext: an item is Cin plaintexts, the result Cout plaintexts.

    definition  out[I](y, x) = b[I] + sum_J sum_dy sum_dx K[I][J][dy][dx] in[J](y + dy - ah, x + dx - aw),  pixels outside the plane = 0
    offsets     t = dy kw + dx, u = dy - ah, v = dx - aw, mask mu_{u,v}[i] = [0 <= y + u < H and 0 <= x + v < W]
    flat        out[I] = sum_J sum_t w^{IJ}_t o rot_{a_t}(in[J]) + b[I],  a_t = (u W + v) mod cols,  w^{IJ}_t[i] = K[I][J][dy][dx] mu_{u,v}[i]
    split       out[I] = sum_dy rot_{(u W) mod cols}( sum_J sum_dx w'^{IJ}_t o rot_{v mod cols}(in[J]) ) + b[I],  w'_t[i] = w_t[(i - u W) mod cols]

Where the mask is 1, i + u W + v stays in the P-block of i, so the cyclic rotation of the whole row does no harm.  A plain module, imported like
linear_grid_model."""
import numpy as np

import bsgs_model as BM

FLAT, SPLIT = 1, 2


def refused(cols, H, W, Cin, Cout, kh, kw, ah, aw, form=0):
    """None, or the word of the condition the shape breaks (the order fhesi_conv2d_plan checks them in)"""
    if cols < 1 or cols > 1 << 20:
        return "outside [1, 2^20]"
    if min(H, W, Cin, Cout, kh, kw) < 1:
        return "at least 1"
    if H * W > cols or cols % (H * W):
        return "does not divide"
    if not (0 <= ah < kh and 0 <= aw < kw):
        return "anchor"
    for dy in range(kh):
        for dx in range(kw):
            u, v = dy - ah, dx - aw
            if abs(u) >= H or abs(v) >= W:
                return f"the offset ({u}, {v}) has an empty mask"
    if Cout * Cin * kh * kw > 65535:
        return "per handle"
    if form not in (0, FLAT, SPLIT):
        return "form"
    return None


def key_switches(Cin, Cout, kh, kw, form):
    return Cin * (kh * kw - 1) if form == FLAT else Cin * (kw - 1) + Cout * (kh - 1)


def offsets(kh, kw, ah, aw):
    """(u, v) of entry t = dy kw + dx"""
    return [(dy - ah, dx - aw) for dy in range(kh) for dx in range(kw)]


def plan(cols, H, W, Cin, Cout, kh, kw, ah, aw, form=0):
    """form 0: the form of fewer key switches, flat on a tie.  amounts in the order the run call takes its matrices"""
    assert refused(cols, H, W, Cin, Cout, kh, kw, ah, aw, form) is None
    if not form:
        form = SPLIT if key_switches(Cin, Cout, kh, kw, SPLIT) < key_switches(Cin, Cout, kh, kw, FLAT) else FLAT
    if form == FLAT:
        amounts = [(u * W + v) % cols for u, v in offsets(kh, kw, ah, aw)]
        terms = Cin * kh * kw
    else:
        amounts = [(dx - aw) % cols for dx in range(kw)] + [((dy - ah) * W) % cols for dy in range(kh)]
        terms = Cin * kw
    return {"form": form, "nh": len(amounts), "key_switches": key_switches(Cin, Cout, kh, kw, form), "terms": terms, "amounts": amounts}


def images(x, H, W, rows):
    """slot values [..][rows * cols] -> [..][rows][cols / P][H][W]"""
    x = np.asarray(x)
    cols = x.shape[-1] // rows
    return x.reshape(x.shape[:-1] + (rows, cols // (H * W), H, W))


def direct(K, bias, xs, H, W, anchor, p, rows):
    """the definition on slot values xs [Cin][rows * cols] -> [Cout][rows * cols] modulo p, every image on its own"""
    K = np.asarray(K, dtype=object)
    Cout, Cin, kh, kw = K.shape
    ah, aw = anchor
    img = np.asarray(images(np.asarray(xs, dtype=object), H, W, rows), dtype=object)      # [Cin][rows][nimg][H][W]
    out = np.zeros((Cout,) + img.shape[1:], dtype=object)
    for I in range(Cout):
        for y in range(H):
            for x in range(W):
                acc = np.zeros(img.shape[1:3], dtype=object) + (0 if bias is None else int(bias[I]))
                for J in range(Cin):
                    for dy in range(kh):
                        for dx in range(kw):
                            yy, xx = y + dy - ah, x + dx - aw
                            if 0 <= yy < H and 0 <= xx < W:
                                acc = acc + int(K[I][J][dy][dx]) * img[J, :, :, yy, xx]
                out[I, :, :, y, x] = acc % p
    return out.reshape(Cout, -1)


def mask(u, v, H, W, rows, cols):
    """mu_{u,v} on every row"""
    i = np.arange(cols) % (H * W)
    y, x = i // W, i % W
    return np.tile(((y + u >= 0) & (y + u < H) & (x + v >= 0) & (x + v < W)).astype(np.int64), rows)


def prepared(K, H, W, anchor, rows, cols, form):
    """[Cout][Cin][kh kw][rows * cols]: w^{IJ}_t (flat) or w'^{IJ}_t (split), entries as they are in K"""
    K = np.asarray(K, dtype=object)
    Cout, Cin, kh, kw = K.shape
    out = np.zeros((Cout, Cin, kh * kw, rows * cols), dtype=object)
    for t, (u, v) in enumerate(offsets(kh, kw, *anchor)):
        mu = np.asarray(mask(u, v, H, W, rows, cols), dtype=object)
        if form == SPLIT:
            mu = BM.rotate_values(mu, -((u * W) % cols), rows)
        for I in range(Cout):
            for J in range(Cin):
                out[I][J][t] = int(K[I][J][t // kw][t % kw]) * mu
    return out


def schedule(K, bias, xs, H, W, anchor, p, rows, form):
    """the schedule of the run call on slot values xs [Cin][rows * cols] -> [Cout][rows * cols] modulo p"""
    K = np.asarray(K, dtype=object)
    Cout, Cin, kh, kw = K.shape
    cols = len(xs[0]) // rows
    pl = plan(cols, H, W, Cin, Cout, kh, kw, anchor[0], anchor[1], form)
    w = prepared(K, H, W, anchor, rows, cols, pl["form"]) % p
    B, G = (kh * kw, 1) if pl["form"] == FLAT else (kw, kh)
    kb, kg = pl["amounts"][:B], ([0] if pl["form"] == FLAT else pl["amounts"][B:])
    babies = [[np.asarray(BM.rotate_values(xs[J], a, rows), dtype=object) for a in kb] for J in range(Cin)]      # once per input channel
    out = []
    for I in range(Cout):
        acc = np.zeros(rows * cols, dtype=object)
        for g in range(G):
            inner = np.zeros(rows * cols, dtype=object)
            for J in range(Cin):
                for j in range(B):
                    inner = (inner + w[I][J][g * B + j] * babies[J][j]) % p
            acc = (acc + BM.rotate_values(inner, kg[g], rows)) % p                                                  # once per output channel
        if bias is not None:
            acc = (acc + int(bias[I])) % p
        out.append(acc)
    return np.stack(out)


def sum_lists(nI, nJ, nk, B, G, cnt):
    """the index lists of the ONE plaintext sum of cnt items (grid_sum_lists, conv_plan.h): group (I G + g) cnt + i, terms (J, j)"""
    nb = min(B, nk)
    a_idx, b_idx, seg = [], [], [0]
    for I in range(nI):
        for g in range(G):
            for i in range(cnt):
                for J in range(nJ):
                    for j in range(B):
                        if g * B + j < nk:
                            a_idx.append((J * nb + j) * cnt + i)
                            b_idx.append((I * nJ + J) * nk + g * B + j)
                seg.append(len(a_idx))
    return a_idx, b_idx, seg


def toeplitz(K, H, W, anchor, p):
    """the same map as a dense matrix [Cout P][Cin P] over one image per channel: row I P + y W + x, column J P + yy W + xx"""
    K = np.asarray(K, dtype=object)
    Cout, Cin, kh, kw = K.shape
    P = H * W
    M = np.zeros((Cout * P, Cin * P), dtype=np.int64)
    for I in range(Cout):
        for J in range(Cin):
            for y in range(H):
                for x in range(W):
                    for dy in range(kh):
                        for dx in range(kw):
                            yy, xx = y + dy - anchor[0], x + dx - anchor[1]
                            if 0 <= yy < H and 0 <= xx < W:
                                M[I * P + y * W + x][J * P + yy * W + xx] = int(K[I][J][dy][dx]) % p
    return M
