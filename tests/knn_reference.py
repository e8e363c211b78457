"""numpy restatement of the k-nearest-neighbour contract of include/mgn_hip.h (mgn_knn_search) and of what is built on it:
``knn`` / ``knn_graph`` (torch_cluster layouts), symmetrise + coalesce (PyG ``to_undirected``), top-k per graph (PyG
``SelectTopK`` + ``topk``) and ``knn_interpolate`` in fp64.  No torch.

The squared distance is fp32 with the contract's operation order, ``((dx*dx) + (dy*dy)) + (dz*dz)``: numpy rounds every
ufunc once and never fuses, so the bits are the kernel's.  Candidates are ordered by ``np.lexsort((index, d2))``."""
import numpy as np

CLAMP = np.float32(1e-16)   # the kernel's constant: 1e-16 rounded to fp32


def squared_distances(y, x):
    """[ny, nx] fp32, exact operation order of the contract"""
    y, x = np.asarray(y, dtype=np.float32), np.asarray(x, dtype=np.float32)
    assert y.shape[1] == x.shape[1] and x.shape[1] in (2, 3)
    d = y[:, None, :] - x[None, :, :]
    s = (d[..., 0] * d[..., 0]) + (d[..., 1] * d[..., 1])
    if x.shape[1] == 3:
        s = s + (d[..., 2] * d[..., 2])
    assert s.dtype == np.float32
    return s


def _first_k(D, k):
    """(d2, column) of the first k entries of every row of D in the order np.lexsort((column, d2)).  On wide rows only the
    entries not above the row's k-th smallest value are ordered (nothing else can be among the first k, ties included): the
    same answer as ordering the whole row, without sorting it."""
    ny, n = D.shape
    if n <= 8 * k:
        col = np.broadcast_to(np.arange(n, dtype=np.int64), D.shape)
        order = np.lexsort((col, D), axis=-1)[:, :k]
        return np.take_along_axis(D, order, axis=1), order
    thr = np.partition(D, k - 1, axis=1)[:, k - 1:k]
    thr = np.where(np.isnan(thr), np.float32(np.inf), thr)
    r, c = np.nonzero(D <= thr)                                   # row-major: columns ascending inside a row
    start = np.searchsorted(r, np.arange(ny))
    width = int(np.bincount(r, minlength=ny).max())
    col = np.full((ny, width), n, dtype=np.int64)                 # padding: behind every real column, at distance +inf
    col[r, np.arange(len(r)) - start[r]] = c
    Dc = np.where(col < n, np.take_along_axis(D, np.minimum(col, n - 1), axis=1), np.float32(np.inf))
    order = np.lexsort((col, Dc), axis=-1)[:, :k]
    return np.take_along_axis(Dc, order, axis=1), np.take_along_axis(col, order, axis=1)


def knn_reference(x, y, k, ptr_x=None, ptr_y=None, exclude_self=False):
    """(idx [ny, k] int64, d2 [ny, k] fp32): nearest first by (d2, global reference index); -1 / +inf where the segment runs out
    of references.  ``exclude_self`` drops the reference whose global index equals the query's.  A reference at a non-finite
    distance is never selected."""
    x, y = np.asarray(x, dtype=np.float32), np.asarray(y, dtype=np.float32)
    nx, ny = x.shape[0], y.shape[0]
    ptr_x = [0, nx] if ptr_x is None else list(ptr_x)
    ptr_y = [0, ny] if ptr_y is None else list(ptr_y)
    assert len(ptr_x) == len(ptr_y)
    idx = np.full((ny, k), -1, dtype=np.int64)
    d2 = np.full((ny, k), np.inf, dtype=np.float32)
    for s in range(len(ptr_x) - 1):
        x0, x1, y0, y1 = ptr_x[s], ptr_x[s + 1], ptr_y[s], ptr_y[s + 1]
        if x1 == x0 or y1 == y0:
            continue
        D = squared_distances(y[y0:y1], x[x0:x1])
        if exclude_self:
            q = np.arange(y0, y1)
            own = (q >= x0) & (q < x1)
            D[np.nonzero(own)[0], q[own] - x0] = np.inf
        dsel, isel = _first_k(D, k)
        isel = isel + x0
        ok = np.isfinite(dsel)
        m = dsel.shape[1]
        idx[y0:y1, :m] = np.where(ok, isel, -1)
        d2[y0:y1, :m] = np.where(ok, dsel, np.float32(np.inf))
    return idx, d2


def assign_index(idx):
    """[2, M] rows (query, reference), grouped by query, nearest first, empty slots removed: torch_cluster.knn's layout"""
    ny, k = idx.shape
    q = np.repeat(np.arange(ny, dtype=np.int64), k)
    r = idx.reshape(-1)
    keep = r >= 0
    return np.stack([q[keep], r[keep]])


def to_undirected(edge_index, num_nodes):
    """both directions of every edge, each pair once, sorted by (row 0, row 1)"""
    row, col = edge_index
    key = np.unique(np.concatenate([row * np.int64(num_nodes) + col, col * np.int64(num_nodes) + row]))
    return np.stack([key // num_nodes, key % num_nodes]).astype(np.int64)


def knn_graph_reference(pos, k, ptr=None, loop=False, flow="source_to_target", force_undirected=False):
    pos = np.asarray(pos, dtype=np.float32)
    idx, _ = knn_reference(pos, pos, k, ptr, ptr, exclude_self=not loop)
    ctr, nbr = assign_index(idx)
    ei = np.stack([nbr, ctr]) if flow == "source_to_target" else np.stack([ctr, nbr])
    return to_undirected(ei, pos.shape[0]) if force_undirected else ei


def num_selected(ratio, n):
    """ceil(ratio * n) in fp32, as PyG's topk computes it"""
    return np.ceil(np.float32(ratio) * np.asarray(n).astype(np.float32)).astype(np.int64)


def topk_reference(score, ratio, ptr):
    """perm: per graph the ceil(ratio * n) highest scores, by graph, then by descending score (ties: lower node first)"""
    score = np.asarray(score)
    out = []
    for g in range(len(ptr) - 1):
        a, b = ptr[g], ptr[g + 1]
        keep = min(int(num_selected(ratio, b - a)), b - a)
        out.append(a + np.argsort(-score[a:b], kind="stable")[:keep])
    return np.concatenate(out).astype(np.int64) if out else np.zeros(0, dtype=np.int64)


def interpolation_weights(idx, d2):
    """a [ny, k] fp64: w / sum w, w = 1 / max(d2, 1e-16), 0 in the empty slots"""
    w = 1.0 / np.maximum(np.asarray(d2, dtype=np.float64), np.float64(CLAMP))
    w = np.where(idx >= 0, w, 0.0)
    tot = w.sum(axis=1, keepdims=True)
    return np.divide(w, tot, out=np.zeros_like(w), where=tot > 0)


def interpolate_reference(x, idx, d2):
    """(out [ny, F] fp64, scale [ny, F] fp64 = sum_j a_j |x[idx_j]|: what the rounding bound is relative to)"""
    x = np.asarray(x, dtype=np.float64)
    a = interpolation_weights(idx, d2)
    rows = x[np.maximum(idx, 0)]                     # [ny, k, F]
    return (a[..., None] * rows).sum(axis=1), (a[..., None] * np.abs(rows)).sum(axis=1)


def interpolate_backward_reference(dy, idx, d2, nx):
    """(dx [nx, F] fp64, scale [nx, F] fp64): the transpose of the interpolation, summed over incoming slots"""
    dy = np.asarray(dy, dtype=np.float64)
    a = interpolation_weights(idx, d2)
    dx, scale = np.zeros((nx, dy.shape[1])), np.zeros((nx, dy.shape[1]))
    yy, jj = np.nonzero(idx >= 0)
    np.add.at(dx, idx[yy, jj], a[yy, jj, None] * dy[yy])
    np.add.at(scale, idx[yy, jj], a[yy, jj, None] * np.abs(dy[yy]))
    return dx, scale
