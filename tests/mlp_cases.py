"""Case table and references of the generic MLP kernels (k_mlp_fwd / k_mlp_bwd behind ops.MlpFunction and the processor
blocks off the packed path).  Shared by tests/test_mlp_cases_host.py (CPU: the references alone stay inside the bars)
and tests/test_hip_mlp_matrix.py (GPU: the engine against them).

Families
  A  build_mlp(fin, H, fout, nb_of_layers, layer_norm, act): widths next to a multiple of 16, rows next to the tile
     edges (a wave owns 16 rows, a workgroup 64), depths 2 .. 8, three activations; at H = 128 the three routes of
     ops.MlpFunction ("full", "enc", "generic").
  B  GraphNetBlock(H, nb_of_layers) off the packed path on a ragged multigraph with a long destination segment.
  C  one block step with more than 131072 edge AND node rows: the MT = 2 instances (32 rows per wave).
  D  stand-alone shapes of A in the bf16 matrix mode (precision = 1 of the generic kernels).

Every reference is computed once per process (``lru_cache``) and handed out detached; callers must not write to it."""
from __future__ import annotations

import functools
from collections import OrderedDict
from dataclasses import dataclass
from typing import Dict, Optional, Tuple

import torch

import recipe as R
from oracle import mgn_oracle as O

FWD_TOL, GRAD_TOL = 1e-5, 1e-4
HS = (16, 32, 64, 128)
ACTS = ("relu", "silu", "gelu")
#: (nb_of_layers, rows).  65 = a workgroup + 1 row, 257 = 4 workgroups + 1, 17 = a tile + 1, 63 = a workgroup - 1
DEPTH_ROWS = ((2, 65), (4, 257), (5, 17), (8, 63), (3, 1))
EXTRA_ROWS = (15, 16, 64)   # on one shape per H
PAD_ROWS = 19               # sentinel rows behind every input / cotangent buffer


def pad16(n: int) -> int:
    return (n + 15) & ~15


def width_pairs(H: int):
    """(fin, fout, masks) of family A at hidden size H.  ``masks``: what the pair is IN the table for, stated by hand and
    checked against the shapes by the host test -- "in"/"out": a 16-block of the input / output is cut by the width (the
    per-element guards of load_tl / store_tl); "inblk"/"outblk": whole 16-blocks are absent (nkb / nib_last of gemm_tl)."""
    wide = H > 16
    pairs = [
        (1, 1, {"in", "out"} | ({"inblk", "outblk"} if wide else set())),
        (3, 2, {"in", "out"} | ({"inblk", "outblk"} if wide else set())),
        (11, 3, {"in", "out"} | ({"inblk", "outblk"} if wide else set())),
        ((15, 17, {"in", "out", "inblk"} | ({"outblk"} if H > 32 else set())) if wide else (15, 15, {"in", "out"})),
        (16, 16, {"inblk", "outblk"} if wide else set()),
        (17, 15, {"in", "out", "outblk"} | ({"inblk"} if H > 32 else set())),
        (H - 1, H - 1, {"in", "out"}),
        (H, 3, {"out"} | ({"outblk"} if wide else set())),
        (H, H, set()),
        (23 if H >= 64 else 11, H, {"in"} | ({"inblk"} if wide else set())),
        (H, H - 1, {"out"}),
    ]
    out, seen = [], set()
    for fin, fout, masks in pairs:
        if fin > H or fout > H or (fin, fout) in seen:   # H = 16: (17, 15) does not exist, (16, 16) = (H, H), (15, 15) = (H-1, H-1)
            continue
        seen.add((fin, fout))
        out.append((fin, fout, frozenset(masks)))
    return out


@dataclass(frozen=True)
class MlpCase:
    fin: int
    H: int
    fout: int
    NL: int
    M: int
    act: str
    norm: bool
    seed: int
    masks: frozenset = frozenset()
    prefix: str = ""

    @property
    def name(self) -> str:
        return f"{self.prefix}h{self.H}_in{self.fin}_out{self.fout}_l{self.NL}_m{self.M}_{self.act}" + ("_norm" if self.norm else "")

    @property
    def wants_dx(self) -> bool:   # the engine differentiates a full-width input only (ops.MlpFunction.backward)
        return self.fin == self.H

    @property
    def route(self) -> str:
        """the launch ops.MlpFunction documents for this shape (its docstring; MGN_FP32_MFMA unset)"""
        if self.H != 128 or self.fout != 128 or self.act == "gelu":
            return "generic"
        if self.fin == 128 and self.NL <= 4:
            return "full"
        if self.fin < 128 and 3 <= self.NL <= 4:
            return "enc"
        return "generic"


def _family_a():
    cases = []
    for hi, H in enumerate(HS):
        norm_turn = 0
        for i, (fin, fout, masks) in enumerate(width_pairs(H)):
            NL, M = DEPTH_ROWS[(i + hi) % 5]
            act = ACTS[(i + 2 * hi) % 3]
            norm = False
            if fout == H:   # layer_norm on alternate cases that can carry one
                norm, norm_turn = norm_turn % 2 == 0, norm_turn + 1
            cases.append(MlpCase(fin, H, fout, NL, M, act, norm, 1000 * (hi + 1) + 10 * i, masks))
        for j, M in enumerate(EXTRA_ROWS):   # three more row counts on (H, H), 4 layers
            cases.append(MlpCase(H, H, H, 4, M, ACTS[(j + hi) % 3], j % 2 == 0, 1000 * (hi + 1) + 500 + 10 * j))
    # the H = 128 routes the cycling above does not reach, stated one by one
    cases += [
        MlpCase(128, 128, 128, 2, 65, "silu", True, 5010),                              # full, SiLU, shortest chain
        MlpCase(128, 128, 128, 3, 1, "relu", False, 5020),                              # full, one row
        MlpCase(11, 128, 128, 4, 257, "relu", True, 5030, frozenset({"in", "inblk"})),  # enc
        MlpCase(23, 128, 128, 3, 17, "silu", False, 5040, frozenset({"in", "inblk"})),  # enc, SiLU
        MlpCase(128, 128, 128, 5, 17, "relu", True, 5050),                              # generic: LDS kernels off above 4 layers
        MlpCase(128, 128, 128, 8, 63, "silu", True, 5060),                              # generic, deepest
        MlpCase(128, 128, 128, 8, 257, "relu", False, 5065),
        MlpCase(11, 128, 128, 2, 65, "relu", True, 5070, frozenset({"in", "inblk"})),   # generic: the enc split is declined
        MlpCase(127, 128, 128, 5, 65, "silu", True, 5080, frozenset({"in"})),           # generic: narrow input, 5 layers
        MlpCase(128, 128, 128, 3, 65, "gelu", False, 5090),                            # generic: GELU
    ]
    names = [c.name for c in cases]
    assert len(set(names)) == len(names), sorted(n for n in names if names.count(n) > 1)
    return OrderedDict((c.name, c) for c in cases)


FAMILY_A: "OrderedDict[str, MlpCase]" = _family_a()


@dataclass(frozen=True)
class BlockCase:
    H: int
    NL: int
    act: str
    N: int
    E: int
    seed: int
    hub: bool = True

    @property
    def name(self) -> str:
        return f"blk_h{self.H}_l{self.NL}_{self.act}_n{self.N}_e{self.E}"


def _family_b():
    cases = []
    k = 0
    for H in (16, 32, 64):
        for NL in (2, 4, 5):
            cases.append(BlockCase(H, NL, ("relu", "silu")[k % 2], 61, 403, 7000 + 10 * k))
            k += 1
    cases += [BlockCase(128, 5, "relu", 61, 403, 7100), BlockCase(128, 8, "silu", 61, 403, 7110)]
    return OrderedDict((c.name, c) for c in cases)


FAMILY_B: "OrderedDict[str, BlockCase]" = _family_b()
MT2_ROWS = 64 * 2048   # plan_mlp: from this many rows a wave of the generic kernels owns two 16-row tiles
FAMILY_C: "OrderedDict[str, BlockCase]" = OrderedDict((c.name, c) for c in (
    BlockCase(32, 4, "relu", MT2_ROWS + 5, MT2_ROWS + 37, 7200, hub=False),
    BlockCase(16, 4, "silu", MT2_ROWS + 5, MT2_ROWS + 37, 7210, hub=False),
))

# bf16 matrix mode (family D).  The engine's forward is held to the explicit fp64 restatement below within TWICE the distance
# of O.bf16_mixed() from it.  Where the two references agree bit for bit (no rounding decision differs: common at these sizes)
# that bar is zero and would ask the engine's fp32 RMSNorm / SiLU for torch's last bit, so the seeds below are those (of
# 8000, 8010, ..) at which the references do differ -- on two different CPUs alike.  Their distance, rel_err / rms_err:
#   h32_in11_out32_relu_norm   2.25e-03 / 1.82e-04      h32_in32_out3_relu   6.72e-04 / 1.20e-04      h64_in64_out64_relu_norm   3.98e-03 / 2.90e-04
#   h128_in128_out3_relu       2.36e-03 / 2.79e-04      h64_in17_out15_relu  1.82e-04 / 1.52e-05      h16_in16_out16_relu        0 / 0
#   h32_in11_out32_silu_norm   3.95e-03 / 2.26e-04      h64_in17_out15_silu  7.67e-04 / 1.37e-04
# (16 -> 16 -> 16: 16 k rounded values, none of 40 seeds makes the references differ; the engine has to match exactly there)
FAMILY_D: "OrderedDict[str, MlpCase]" = OrderedDict((c.name, c) for c in (
    MlpCase(11, 32, 32, 4, 257, "relu", True, 8160, prefix="bf16_"),
    MlpCase(32, 32, 3, 4, 257, "relu", False, 8120, prefix="bf16_"),
    MlpCase(64, 64, 64, 4, 257, "relu", True, 8170, prefix="bf16_"),
    MlpCase(128, 128, 3, 4, 257, "relu", False, 8200, prefix="bf16_"),
    MlpCase(17, 64, 15, 4, 257, "relu", False, 8120, prefix="bf16_"),
    MlpCase(16, 16, 16, 4, 257, "relu", False, 8050, prefix="bf16_"),
    MlpCase(11, 32, 32, 4, 257, "silu", True, 8140, prefix="bf16_"),
    MlpCase(17, 64, 15, 4, 257, "silu", False, 8010, prefix="bf16_"),
))


# ------------------------------------------------------------------------------------------------ inputs
def mlp_shapes(fin: int, H: int, fout: int, NL: int, norm: bool, prefix: str = "") -> "OrderedDict[str, Tuple[int, ...]]":
    """state_dict keys / shapes of build_mlp(fin, H, fout, NL, norm): Linear entries 0, 2, .., RMSNorm entry 2 NL - 1"""
    dims = [fin] + [H] * (NL - 1) + [fout]
    sh: "OrderedDict[str, Tuple[int, ...]]" = OrderedDict()
    for l in range(NL):
        sh[f"{prefix}{2 * l}.weight"], sh[f"{prefix}{2 * l}.bias"] = (dims[l + 1], dims[l]), (dims[l + 1],)
    if norm:
        sh[f"{prefix}{2 * NL - 1}.scale"] = (fout,)
    return sh


def block_shapes(H: int, NL: int) -> "OrderedDict[str, Tuple[int, ...]]":
    sh = mlp_shapes(3 * H, H, H, NL, True, "edge_block.")
    sh.update(mlp_shapes(2 * H, H, H, NL, True, "node_block."))
    return sh


def mlp_inputs(c: MlpCase):
    """(params, x[M, fin], cotangent[M, fout])"""
    return (R.make_params(mlp_shapes(c.fin, c.H, c.fout, c.NL, c.norm), c.seed),
            R.randn((c.M, c.fin), c.seed + 1), R.randn((c.M, c.fout), c.seed + 2))


def block_graph(c: BlockCase) -> torch.Tensor:
    """recipe.random_graph (duplicates, a self loop, isolated last node); ``hub``: 120 edges rewired onto one destination"""
    ei = R.random_graph(c.N, c.E, c.seed + 5).clone()
    if c.hub:
        ei[1, 100:220] = 7
    return ei


def block_inputs(c: BlockCase):
    """(params, edge_index, x[N, H], e[E, H], cotangent of x', cotangent of e')"""
    return (R.make_params(block_shapes(c.H, c.NL), c.seed), block_graph(c), R.randn((c.N, c.H), c.seed + 1),
            R.randn((c.E, c.H), c.seed + 2), R.randn((c.N, c.H), c.seed + 3), R.randn((c.E, c.H), c.seed + 4))


# -------------------------------------------------------------------------------------------- references
@dataclass(frozen=True)
class Ref:
    out: Tuple[torch.Tensor, ...]          # forward result(s)
    grads: Dict[str, torch.Tensor]         # by state_dict key
    dins: Tuple[Optional[torch.Tensor], ...]   # input gradient(s); None where the engine has none


def _find(name: str):
    for fam in (FAMILY_A, FAMILY_B, FAMILY_C, FAMILY_D):
        if name in fam:
            return fam[name]
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def reference(name: str, dtype: torch.dtype, mixed: bool = False) -> Ref:
    """the oracle's forward and every gradient of a case in ``dtype`` (``mixed``: under O.bf16_mixed())"""
    c = _find(name)
    if isinstance(c, MlpCase):
        p, x, cot = mlp_inputs(c)
        po = {k: v.to(dtype).requires_grad_(True) for k, v in p.items()}
        xo = x.to(dtype).requires_grad_(True)
        if mixed:
            with O.bf16_mixed():
                y = O.mlp(xo, po, "", c.act)
        else:
            y = O.mlp(xo, po, "", c.act)
        (y * cot.to(dtype)).sum().backward()
        return Ref((y.detach(),), {k: v.grad for k, v in po.items()}, (xo.grad if c.wants_dx else None,))
    p, ei, x, e, cx, ce = block_inputs(c)
    po = {k: v.to(dtype).requires_grad_(True) for k, v in p.items()}
    xo, eo = x.to(dtype).requires_grad_(True), e.to(dtype).requires_grad_(True)
    x2, e2 = O.graph_net_block(xo, eo, ei, po, "", c.act)
    ((x2 * cx.to(dtype)).sum() + (e2 * ce.to(dtype)).sum()).backward()
    return Ref((x2.detach(), e2.detach()), {k: v.grad for k, v in po.items()}, (xo.grad, eo.grad))


def _bf16(t: torch.Tensor) -> torch.Tensor:
    return t.to(torch.float32).to(torch.bfloat16).to(torch.float64)


@functools.lru_cache(maxsize=None)
def bf16_explicit_forward(name: str) -> torch.Tensor:
    """the bf16 matrix mode of a stand-alone MLP restated in fp64: operands (rows, weights, biases) rounded to bf16, fp64
    products and sums, every Linear's result rounded to bf16, a smooth activation's result rounded to bf16 (ReLU of a bf16
    value is exact), the RMSNorm in fp32 on the bf16 result"""
    c = _find(name)
    p, x, _ = mlp_inputs(c)
    f = {"relu": torch.relu, "silu": torch.nn.functional.silu, "gelu": torch.nn.functional.gelu}[c.act]
    h = _bf16(x)
    for l in range(c.NL):
        h = _bf16(h @ _bf16(p[f"{2 * l}.weight"]).t() + _bf16(p[f"{2 * l}.bias"]))
        if l != c.NL - 1:
            h = f(h) if c.act == "relu" else _bf16(f(h))
    h = h.to(torch.float32)
    return O.rms_norm(h, p[f"{2 * c.NL - 1}.scale"]) if c.norm else h


def padded(t: torch.Tensor, fill: float = float("nan")) -> torch.Tensor:
    """``t`` as the leading rows of a larger buffer whose other rows hold ``fill``: a kernel that reads a row past the last
    one (instead of clamping to it) picks the sentinel up"""
    big = torch.full((t.shape[0] + PAD_ROWS,) + tuple(t.shape[1:]), fill, dtype=t.dtype, device=t.device)
    big[:t.shape[0]] = t
    return big[:t.shape[0]]
