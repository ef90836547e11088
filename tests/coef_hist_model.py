"""A numpy model of jsnoop_batch_pack_coef_hist: one row per (image, component) from the tensor coef_model.coef_tensor gives for it in
BLOCKS / I16 / NATURAL.  It is the definition of include/jsnoop_gpu.h and nothing else: plain indexing and np.add.at, no cleverness.

x = v (quantised false) or v / max(q[k], 1), C division truncating toward zero, of the int16 as it stands; position p is natural index p, or
natural index ZIGZAG[p]; hist[p][clamp(x, -R, R) + R] counts blocks; min[p] / max[p] are the extremes of the unclamped x."""
import numpy as np

import coef_model as M


def words(R):
    return 64 * (2 * R + 1) + 128


def levels(tensor, q, quantised):
    """[blocks][64] int64 in natural order: the x of every element of a [bh][bw][64] int16 tensor."""
    v = np.asarray(tensor).reshape(-1, 64).astype(np.int64)
    if not quantised:
        return v
    d = np.maximum(np.asarray(q, np.int64).reshape(64), 1)
    return np.sign(v) * (np.abs(v) // d)


def row_of_tensor(tensor, q, R, quantised=True, zigzag=False):
    assert 1 <= R <= 127
    x = levels(tensor, q, quantised)
    if zigzag:
        x = x[:, M.ZIGZAG]
    nb = 2 * R + 1
    hist = np.zeros((64, nb), np.uint32)
    pos = np.broadcast_to(np.arange(64), x.shape)
    np.add.at(hist, (pos, np.clip(x, -R, R) + R), 1)
    row = np.empty(words(R), np.uint32)
    row[:64 * nb] = hist.reshape(-1)
    row[64 * nb:64 * nb + 64] = x.min(0).astype(np.int32).view(np.uint32)
    row[64 * nb + 64:] = x.max(0).astype(np.int32).view(np.uint32)
    return row


def row(blocks, cum, geo, c, q, R, quantised=True, zigzag=False):
    """The row of component c of one image: blocks [n][64] in decode order, cum the cumulative DC per block, q the 64 DQT entries in natural order."""
    return row_of_tensor(M.coef_tensor(blocks, cum, geo, c), q, R, quantised, zigzag)


def fields(r, R):
    nb = 2 * R + 1
    return r[:64 * nb].reshape(64, nb), r[64 * nb:64 * nb + 64].view(np.int32), r[64 * nb + 64:].view(np.int32)
