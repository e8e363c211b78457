"""fp64 restatement of the Simulator boundary, in numpy only: ``Simulator._build_input_graph`` / ``build_outputs``
(graphphysics/models/simulator.py:80-191), ``Normalizer`` (models/layers.py:281-391) and the rollout's re-imposition of
the ground truth (training/lightning_module.py:27-35).  Written from the reference's text, independent of
``oracle/mgn_oracle.py`` and of the engine; ``tests/golden/simulator_io.npz`` (minted from the unmodified reference)
anchors it, ``tests/test_sim_reference_host.py`` checks that.

What it pins down:
  * ``Normalizer.forward`` accumulates BEFORE it normalises, and only while ``num_accumulations < max_accumulations``;
  * ``mean = sum / max(count, 1)``, ``std = max(sqrt(max(sumsq / max(count, 1) - mean^2, 0)), eps)`` with eps the fp32
    rounding of 1e-8 (the reference holds it in a float32 tensor);
  * the one-hot truncates the float type toward zero (``.long()``) and raises outside [0, 9);
  * the rollout mask COMPARES THE FLOAT: a type of 0.5 is neither NORMAL nor OUTFLOW;
  * arbitrary column windows (``Layout``), ``y`` wider than the output window reads its first O columns.

Also the inputs the simulator tests share (``make_inputs``): every value a multiple of 1/8 in [-2, 2], from an integer
hash (no generator state, the same numbers everywhere), so that every partial sum and sum of squares of every stream
is exactly representable in fp32 in any summation order (``exactly_summable`` states the bound), and sign-balanced so
that no column's mean exceeds its spread (``balanced``).
"""
from dataclasses import dataclass
from typing import Optional

import numpy as np

NODE_TYPES = 9
NODE_NORMAL, NODE_OBSTACLE, NODE_OUTFLOW = 0.0, 1.0, 5.0
STD_EPS = float(np.float32(1e-8))


@dataclass(frozen=True)
class Layout:
    name: str
    x_w: int
    feat_start: int
    feat_end: int
    type_idx: int
    out_start: int
    out_end: int
    y_w: int
    edge_w: int        # edge_input_size; 0 = no edge normaliser
    edge_attr_w: int   # width of the edge_attr tensor handed in (untouched when edge_w == 0)

    @property
    def Wn(self):
        return (self.feat_end - self.feat_start) + NODE_TYPES

    @property
    def O(self):
        return self.out_end - self.out_start

    def sim_kwargs(self):
        return dict(node_input_size=self.Wn, edge_input_size=self.edge_w, output_size=self.O, feature_index_start=self.feat_start,
                    feature_index_end=self.feat_end, output_index_start=self.out_start, output_index_end=self.out_end,
                    node_type_index=self.type_idx)


LAYOUTS = {
    # widest node and edge streams (32 = the fused kernels' column limit), windows away from column 0, y wider than O
    "A": Layout("A", 40, 5, 28, 2, 30, 33, 5, 32, 32),
    # no feature columns, one output column, no edge normaliser (edge_attr passes through)
    "B": Layout("B", 40, 7, 7, 0, 3, 4, 1, 0, 3),
    # the shipped cylinder layout: x = [v_x, v_y, node_type, t]
    "C": Layout("C", 4, 0, 2, 2, 0, 2, 2, 3, 3),
    # widest output stream: N * O sizes the normalising launch
    "E": Layout("E", 40, 4, 4, 1, 8, 40, 32, 1, 1),
    # one column more than the fused kernels take
    "W33": Layout("W33", 40, 5, 29, 2, 30, 33, 3, 3, 3),
}

ROWS = ((1, 0), (7, 9), (8, 8), (9, 7), (2047, 2049), (2048, 2048), (2049, 2047), (4099, 300), (300, 4099))


# ------------------------------------------------------------------------------------------------ inputs
def _hash(r, c, salt):
    """32-bit integer mix of (row, column, salt): numpy uint64 arithmetic masked to 32 bits"""
    M = np.uint64(0xFFFFFFFF)
    h = (r.astype(np.uint64) * np.uint64(2654435761) + c.astype(np.uint64) * np.uint64(40503) + np.uint64(salt) * np.uint64(1234577)) & M
    h ^= h >> np.uint64(15)
    h = (h * np.uint64(2246822519)) & M
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(3266489917)) & M
    h ^= h >> np.uint64(16)
    return h


def eighths(rows: int, cols: int, salt: int) -> np.ndarray:
    """[rows, cols] float32, multiples of 1/8 in [-2, 2]"""
    r, c = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    return ((_hash(r, c, salt) % np.uint64(33)).astype(np.int64) - 16).astype(np.float32) / np.float32(8)


def type_codes(rows: int, salt: int) -> np.ndarray:
    """node-type codes 0..8; the first nine rows hold every code once (all nine present once rows >= 9)"""
    r = np.arange(rows)
    t = (_hash(r, np.zeros_like(r), salt + 7919) % np.uint64(NODE_TYPES)).astype(np.int64)
    k = min(rows, NODE_TYPES)
    t[:k] = (np.arange(k) + salt) % NODE_TYPES
    return t.astype(np.float32)


def balanced(rows: int, cols: int, salt: int, call: int) -> np.ndarray:
    """[rows, cols] multiples of 1/8 in [-2, 2] whose column means stay below the column's spread at EVERY row count:
    rows 2k and 2k + 1 hold v and -v; the last row of an odd count holds the same magnitudes in every call, with the
    sign alternating from call to call.  Then, after any number of calls, |mean| <= std in every column that varies
    (``Normalizer64.well_conditioned``): for one row because the signs alternate, for more because at most one row
    per call is unpaired."""
    out = np.empty((rows, cols), dtype=np.float32)
    half = eighths(rows // 2, cols, salt + 10 * call)
    out[0:2 * (rows // 2):2], out[1:2 * (rows // 2):2] = half, -half
    if rows % 2:
        out[-1] = eighths(1, cols, salt + 5)[0] * np.float32(1 if call % 2 == 0 else -1)
    return out


def make_inputs(lay: Layout, N: int, E: int, call: int, seed: int = 0):
    """(x [N, x_w], y [N, y_w], edge_attr [E, edge_attr_w]) of training / eval call number ``call``"""
    salt = 1000 * seed
    x = balanced(N, lay.x_w, salt + 1, call)
    x[:, lay.type_idx] = type_codes(N, salt + 10 * call)
    return x, balanced(N, lay.y_w, salt + 2, call), balanced(E, lay.edge_attr_w, salt + 3, call)


def case_seed(layout: str, N: int) -> int:
    """the ``seed`` of ``make_inputs`` every test and the golden file use for a layout at N rows"""
    return list(LAYOUTS).index(layout) + 10 * (N > 100)


def mask_types(types: np.ndarray) -> np.ndarray:
    """the type column with non-integral codes sprinkled in for the rollout mask: 0.5 / -0.5 (truncate to NORMAL) and
    5.5 (truncates to OUTFLOW) must all receive the ground truth; NORMAL and OUTFLOW rows next to them keep the prediction"""
    t = np.array(types, dtype=np.float32)
    i = np.arange(t.shape[0])
    t[i % 7 == 0], t[i % 7 == 2] = 0.0, 5.0
    t[i % 7 == 1], t[i % 7 == 3], t[i % 7 == 5] = 0.5, -0.5, 5.5
    return t


def sample_rows(M: int) -> np.ndarray:
    """the rows of an [M, w] tensor the golden file keeps: all of a small one; of a large one the first 4, the last 5
    (both sides of row 2048 at M = 2049) and every 293rd between"""
    if M <= 32:
        return np.arange(M)
    return np.concatenate([np.arange(4), np.arange(4, M - 5, 293), np.arange(M - 5, M)])


def exactly_summable(max_rows: int, calls: int) -> bool:
    """Values are k/8 with |k| <= 16, deltas y - x are k/8 with |k| <= 32: a sum of n of them is an integer multiple of
    1/8 below 4n, a sum of squares an integer multiple of 1/64 below 16n.  Both are fp32 numbers (and so is every partial
    sum, in any order) while 16 n * 64 <= 2^24."""
    return 16 * max_rows * calls * 64 <= 2 ** 24


# ------------------------------------------------------------------------------------------------ restatement
class Normalizer64:
    def __init__(self, size: int, max_accumulations: int = 10 ** 5, eps: float = STD_EPS):
        self.max_accumulations, self.eps = max_accumulations, eps
        self.acc_sum = np.zeros((1, size), dtype=np.float64)
        self.acc_sum_squared = np.zeros((1, size), dtype=np.float64)
        self.acc_count = 0.0
        self.num_accumulations = 0.0

    def load(self, acc_sum, acc_sum_squared, acc_count, num_accumulations):
        self.acc_sum = np.asarray(acc_sum, dtype=np.float64).reshape(1, -1).copy()
        self.acc_sum_squared = np.asarray(acc_sum_squared, dtype=np.float64).reshape(1, -1).copy()
        self.acc_count, self.num_accumulations = float(acc_count), float(num_accumulations)

    def buffers(self):
        return dict(_acc_sum=self.acc_sum.copy(), _acc_sum_squared=self.acc_sum_squared.copy(),
                    _acc_count=np.float64(self.acc_count), _num_accumulations=np.float64(self.num_accumulations))

    def mean(self):
        return self.acc_sum / max(self.acc_count, 1.0)

    def variance(self):
        return self.acc_sum_squared / max(self.acc_count, 1.0) - self.mean() ** 2

    def std(self):
        return np.maximum(np.sqrt(np.maximum(self.variance(), 0.0)), self.eps)

    def __call__(self, v, accumulate: bool):
        v = np.asarray(v, dtype=np.float64)
        if accumulate and self.num_accumulations < self.max_accumulations:
            self.acc_sum += v.sum(axis=0, keepdims=True)
            self.acc_sum_squared += (v ** 2).sum(axis=0, keepdims=True)
            self.acc_count += v.shape[0]
            self.num_accumulations += 1
        return (v - self.mean()) / self.std()

    def inverse(self, v):
        return np.asarray(v, dtype=np.float64) * self.std() + self.mean()

    def well_conditioned(self) -> bool:
        """|mean| <= std in every column that varies: then ``sumsq / count - mean^2`` loses at most one bit to
        cancellation and a 1e-6 bound on an fp32 evaluation is not spent on it.  A column that does not vary has
        variance exactly 0 in fp32 too (its sums are exact), so nothing cancels there either."""
        var, mean = self.variance(), self.mean()
        return bool(np.all((var == 0.0) | (np.abs(mean) <= np.sqrt(np.maximum(var, 0.0)))))


def one_hot(types) -> np.ndarray:
    """F.one_hot(node_type.long(), 9): truncation toward zero, codes outside [0, 9) raise"""
    t = np.trunc(np.asarray(types, dtype=np.float64)).astype(np.int64)
    if t.size and (t.min() < 0 or t.max() >= NODE_TYPES):
        raise RuntimeError("class values must be smaller than num_classes / non-negative")
    return (t[:, None] == np.arange(NODE_TYPES)[None, :]).astype(np.float64)


def keep_mask(types) -> np.ndarray:
    """rows whose prediction stands: the FLOAT type equals NORMAL or OUTFLOW"""
    t = np.asarray(types)
    return (t == NODE_NORMAL) | (t == NODE_OUTFLOW)


class Simulator64:
    def __init__(self, lay: Layout, max_accumulations: int = 10 ** 5):
        self.lay = lay
        self.node = Normalizer64(lay.Wn, max_accumulations)
        self.out = Normalizer64(lay.O, max_accumulations)
        self.edge = Normalizer64(lay.edge_w, max_accumulations) if lay.edge_w > 0 else None

    def norms(self):
        return {"_node_normalizer": self.node, "_output_normalizer": self.out, "_edge_normalizer": self.edge}

    def packed_buffers(self) -> np.ndarray:
        """node, output, edge (if any) normaliser, each [sum (W), sum of squares (W), count, number of accumulations]"""
        return np.concatenate([np.concatenate([n.acc_sum.reshape(-1), n.acc_sum_squared.reshape(-1), [n.acc_count, n.num_accumulations]])
                               for n in (self.node, self.out, self.edge) if n is not None])

    def well_conditioned(self) -> bool:
        return all(n.well_conditioned() for n in (self.node, self.out, self.edge) if n is not None)

    def node_features(self, x):
        lay = self.lay
        return np.concatenate([np.asarray(x, dtype=np.float64)[:, lay.feat_start:lay.feat_end], one_hot(x[:, lay.type_idx])], axis=1)

    def target_delta(self, x, y):
        lay = self.lay
        return np.asarray(y, dtype=np.float64)[:, :lay.O] - np.asarray(x, dtype=np.float64)[:, lay.out_start:lay.out_end]

    def build_input(self, x, y, edge_attr, training: bool):
        """(node features, target, edge features), normalised; the order of the reference: target, nodes, edges"""
        tgt = self.out(self.target_delta(x, y), training) if y is not None else None
        xn = self.node(self.node_features(x), training)
        en = self.edge(edge_attr, training) if self.edge is not None else edge_attr
        return xn, tgt, en

    def build_outputs(self, x, net_out):
        lay = self.lay
        return np.asarray(x, dtype=np.float64)[:, lay.out_start:lay.out_end] + self.out.inverse(net_out)

    def predict(self, x, y, net_out, mask_truth: bool, types: Optional[np.ndarray] = None):
        pred = self.build_outputs(x, net_out)
        if mask_truth:
            t = x[:, self.lay.type_idx] if types is None else types
            pred = np.where(keep_mask(t)[:, None], pred, np.asarray(y, dtype=np.float64)[:, :self.lay.O])
        return pred


def rel_err(a, b) -> float:
    """max |a - b| / max |b|, in fp64"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.size == 0:
        return 0.0
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))
