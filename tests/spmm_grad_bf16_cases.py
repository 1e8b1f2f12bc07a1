"""The order of the sum of the wide-batch value gradient with bf16 activations (hispmv_spmm_value_grad_device_bf16), as a numpy float32
model -- no device, no library call except the host tile rule.

Per entry and tile of 64 * VB vectors: the products of the tile as float32 (one rounding each; the product of a vector past the batch is
+0), reshaped to [64 lanes, VB]; summed sequentially from +0 along VB; then six rounds of s[0::2] + s[1::2] (the pairwise tree over the
lanes); then alpha * s (+ beta * grad for the first tile, + grad for every later one) in float32 operations, tiles ascending.  With VB in
{4, 2, 1} and the tiles of prep.spmm_tiles the same model is the fp32 entry's order (hispmv_spmm_value_grad_device)."""
import numpy as np


def to_bf16_bits(a):
    """float32 -> the bf16 bits (uint16): nearest, ties to even; NaN stays NaN (quiet), +-Inf stay"""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32)
    r = ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)
    nan = (u & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)
    return np.where(nan, ((u >> np.uint32(16)) | np.uint32(0x40)).astype(np.uint16), r)


def widen(a16):
    """bf16 bits -> float32, exact"""
    return (np.ascontiguousarray(a16, np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def tile_list(tiles, key="vb"):
    """prep.spmm_bf16_tiles(...) (or prep.spmm_tiles with key="vl") -> [(first vector, vectors, lane width)]: every tile but the last is
    full and has the first tile's width"""
    out, k = [], 0
    for t in range(tiles["tiles"]):
        last = t == tiles["tiles"] - 1
        w = tiles[key + "_last"] if last else tiles[key]
        n = tiles["last_vecs"] if last else 64 * w
        out.append((k, n, w))
        k += n
    return out


def tile_sum(gy, x, vb):
    """gy, x: float32 [n, vecs of the tile <= 64 * vb] -> float32 [n], the sum of one tile in the kernel's order"""
    n, nv = gy.shape
    assert nv <= 64 * vb and x.shape == gy.shape
    with np.errstate(invalid="ignore", over="ignore"):
        p = np.zeros((n, 64 * vb), np.float32)
        p[:, :nv] = gy.astype(np.float32) * x.astype(np.float32)
        p = p.reshape(n, 64, vb)
        s = np.zeros((n, 64), np.float32)
        for i in range(vb):
            s = s + p[:, :, i]
        for _ in range(6):
            s = s[:, 0::2] + s[:, 1::2]
    return s[:, 0]


def model(gy, x, tiles, alpha, beta, grad0=None):
    """gy = gyt[row_k, :B], x = xt[col_k, :B] as float32 [n, B]; tiles from tile_list; -> grad float32 [n].  alpha == 0 is the in-place
    prologue: exactly beta * grad0, or +0."""
    n = gy.shape[0]
    alpha, beta = np.float32(alpha), np.float32(beta)
    g = np.zeros(n, np.float32) if grad0 is None else np.asarray(grad0, np.float32).copy()
    with np.errstate(invalid="ignore", over="ignore"):
        if alpha == 0:
            return beta * g if beta != 0 else np.zeros(n, np.float32)
        for t, (k0, nv, vb) in enumerate(tiles):
            r = alpha * tile_sum(gy[:, k0:k0 + nv], x[:, k0:k0 + nv], vb)
            b = beta if t == 0 else np.float32(1.0)
            g = r + b * g if b != 0 else r
    return g
