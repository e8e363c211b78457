#!/usr/bin/env python3
"""Mint ``mtp.npz`` from the REFERENCE implementation (build container only).

Run:  python tests/golden/make_golden_mtp.py            (needs the reference checkout)

The reference's ``graphphysics/models/spatial_mtp_1hop.py`` and ``build_mlp`` (the shared output head) are imported unmodified,
with the stand-ins of make_golden.py.  Only arrays and name lists leave this script.

The mesh of every case: 40 nodes; a ring over nodes 0..37, the chords 0-10 and 0-20, a self loop 5-5 and the edge 5-6 two more
times, every pair in both directions (so the self loop is there twice); nodes 38 and 39 are isolated.

Cases (``<case>.<name>`` in the file; every case carries its own inputs):
  messy          centres [0, 5, 39, 6, 12] (16 pairs, max_deg 6), d = 32, 4 heads, 2 layers, O = 2, reduction "mean_per_center"
  messy_mean     the same with reduction "mean"
  messy_noneigh  the same with H_neigh = None
  messy_rowptr   the same with row_ptr / dst_sorted given (stored)
  directed       the pairs in ONE direction with assume_undirected = False; d = 16, 1 head, 1 layer
  isolated       centres [39]
  empty          no centres
Per case: ``meta`` = [d, heads, layers, O, assume_undirected, has H_neigh, has row_ptr, reduction is "mean"], H, H_neigh, edge_index,
centers, target, every weight of the module (``w.<key>``) and of the head ``build_mlp(d, d, O, layer_norm=False)`` (``head.<key>``);
then for the fp32 run (``f32.``) and for the same module and inputs in ``.double()`` (``f64.``): ``loss``, ``stat.<name>`` for every
stat, and the gradients ``g.H``, ``g.H_neigh``, ``g.w.<key>``, ``g.head.<key>`` (none where the loss is the constant zero).
Every d = 32 case shares the inputs and weights of ``messy`` (asserted here; the weights are stored once, under ``messy``).  The
matrix gradients of the three variants of ``messy`` are stored as the other block goldens store them, to keep the file small: the first 8 rows
(``<key>__rows8``) and the Frobenius norm (``<key>__norm``); vectors and the input gradients are stored whole.
``state_keys`` / ``state_shapes``: the sorted ``state_dict`` keys of a 2-layer module and their shapes (padded with zeros to 2)."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)

import make_golden as MG  # noqa: E402

N_NODES = 40


def mesh_pairs():
    pairs = [(i, (i + 1) % 38) for i in range(38)] + [(0, 10), (0, 20), (5, 5), (5, 6), (5, 6)]
    return np.array(pairs, dtype=np.int64).T


def mesh_edges(directed=False):
    p = mesh_pairs()
    return p if directed else np.concatenate([p, p[::-1]], axis=1)


CASES = {
    "messy": dict(centers=[0, 5, 39, 6, 12], d=32, heads=4, layers=2, O=2),
    "messy_mean": dict(centers=[0, 5, 39, 6, 12], d=32, heads=4, layers=2, O=2, reduction="mean"),
    "messy_noneigh": dict(centers=[0, 5, 39, 6, 12], d=32, heads=4, layers=2, O=2, neigh=False),
    "messy_rowptr": dict(centers=[0, 5, 39, 6, 12], d=32, heads=4, layers=2, O=2, rowptr=True),
    "directed": dict(centers=[0, 5, 6, 20, 39, 10], d=16, heads=1, layers=1, O=2, directed=True),
    "isolated": dict(centers=[39], d=32, heads=4, layers=2, O=2),
    "empty": dict(centers=[], d=32, heads=4, layers=2, O=2),
}


def main():
    if not os.path.isdir(MG.REF):
        sys.exit("reference checkout not present: goldens can only be minted in the build container")
    MG.install_standins()
    torch.set_num_threads(4)
    from graphphysics.models.layers import build_mlp as ref_build_mlp
    from graphphysics.models.spatial_mtp_1hop import SpatialMTP1Hop as RefMTP, _sorted_by_src

    out = {}
    for ci, (name, c) in enumerate(CASES.items()):
        d, heads, layers, O = c["d"], c["heads"], c["layers"], c["O"]
        directed, neigh, rowptr = c.get("directed", False), c.get("neigh", True), c.get("rowptr", False)
        reduction = c.get("reduction", "mean_per_center")
        seed = 4100 if d == 32 else 4200 + ci    # every d = 32 case shares the inputs and weights of messy
        torch.manual_seed(seed)
        mod = RefMTP(d, num_heads=heads, num_layers=layers, assume_undirected=not directed)
        head = ref_build_mlp(d, d, O, layer_norm=False)
        g = torch.Generator().manual_seed(seed + 1)
        with torch.no_grad():   # off the initialisers' special values (ones, zeros): every parameter's gradient path counts
            for p in list(mod.parameters()) + list(head.parameters()):
                p.add_(0.1 * torch.randn(p.shape, generator=g))
        H = torch.randn(N_NODES, d, generator=g)
        Hn = torch.randn(N_NODES, d, generator=g)
        target = torch.randn(N_NODES, O, generator=g)
        ei = torch.from_numpy(mesh_edges(directed))
        centers = torch.tensor(c["centers"], dtype=torch.long)
        pre = name + "."
        out[pre + "meta"] = np.array([d, heads, layers, O, int(not directed), int(neigh), int(rowptr), int(reduction == "mean")], dtype=np.int64)
        out.update({pre + "H": H.numpy(), pre + "H_neigh": Hn.numpy(), pre + "target": target.numpy(), pre + "edge_index": ei.numpy(),
                    pre + "centers": centers.numpy()})
        variant = name.startswith("messy_")
        shared = d == 32 and name != "messy"
        for k, v in list(("w." + k, v) for k, v in mod.state_dict().items()) + list(("head." + k, v) for k, v in head.state_dict().items()):
            if shared:
                assert np.array_equal(out["messy." + k], v.detach().numpy()), k
            else:
                out[pre + k] = v.detach().clone().numpy()
        kw = {}
        if rowptr:
            _, dst_s, rp = _sorted_by_src(ei, N_NODES)
            kw = dict(row_ptr=rp, dst_sorted=dst_s)
            out[pre + "row_ptr"], out[pre + "dst_sorted"] = rp.numpy(), dst_s.numpy()
        for tag, dt in (("f32.", torch.float32), ("f64.", torch.float64)):
            m, h = mod.to(dt), head.to(dt)
            for p in list(m.parameters()) + list(h.parameters()):
                p.grad = None
            Hx, Hnx = H.to(dt).clone().requires_grad_(True), Hn.to(dt).clone().requires_grad_(True)
            loss, stats = m(Hx, ei, centers, h, target.to(dt), reduction=reduction, H_neigh=Hnx if neigh else None, **kw)
            out[pre + tag + "loss"] = loss.detach().numpy()
            for k, v in stats.items():
                out[pre + tag + "stat." + k] = v.detach().numpy()
            if loss.requires_grad:
                loss.backward()
                out[pre + tag + "g.H"] = Hx.grad.numpy()
                if neigh:
                    out[pre + tag + "g.H_neigh"] = Hnx.grad.numpy()
                for k, p in [("w." + k, p) for k, p in m.named_parameters()] + [("head." + k, p) for k, p in h.named_parameters()]:
                    if variant and p.dim() == 2:
                        out[pre + tag + "g." + k + "__rows8"] = p.grad[:8].numpy().copy()
                        out[pre + tag + "g." + k + "__norm"] = p.grad.norm().numpy().copy()
                    else:
                        out[pre + tag + "g." + k] = p.grad.numpy().copy()
        if name == "messy":
            assert float(stats["sp_mtp/pairs"]) == 16 and float(stats["sp_mtp/max_deg"]) == 6, stats
        mod.to(torch.float32), head.to(torch.float32)
    sd = RefMTP(32, num_heads=4, num_layers=2).state_dict()
    keys = sorted(sd)
    out["state_keys"] = np.array(keys)
    out["state_shapes"] = np.array([list(sd[k].shape) + [0] * (2 - sd[k].dim()) for k in keys], dtype=np.int64)
    path = os.path.join(HERE, "mtp.npz")
    np.savez_compressed(path, **out)
    print(f"wrote mtp.npz  ({os.path.getsize(path) / 1024:.0f} kB, {len(out)} arrays)")


if __name__ == "__main__":
    main()
