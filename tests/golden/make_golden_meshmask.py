#!/usr/bin/env python3
"""Mint ``meshmask.npz`` from the REFERENCE implementation (build container only).

Run:  python tests/golden/make_golden_meshmask.py            (needs the reference checkout)

The reference's ``utils/meshmask.py``, ``utils/torch_graph.get_masked_indexes`` and ``utils/loss.py`` are imported unmodified,
with the stand-ins of make_golden.py (loguru, torch_geometric) plus ``torch_geometric.utils.num_nodes.maybe_num_nodes``
(``edge_index.max() + 1``, what torch-geometric 2.6.1 returns for a tensor and ``num_nodes=None``) and empty modules for what
``torch_graph`` imports at its top and ``get_masked_indexes`` never touches (meshio, torch_geometric.transforms / .loader).
``meshmask.device`` and ``loss.device`` are set to the CPU.  Only arrays leave this script.

Cases (each carries its own inputs):
  messy   the mesh of make_golden_losses.py (unsorted ``edge_index`` with duplicates, one-directional edges and a self loop),
          150 nodes, a seeded unsorted selection of 127 of them
  grid    ``loss_cases.grid2d(7, 9, 300)``: 63 nodes, a fixed unsorted selection of 40
Per case: x [N, 5], pos, edge_attr [E, 3], the selection, the latent tensors (k x 6 / E' x 4), both tokens, the edge encoder's
weight and bias (one Linear 3 -> 4) and the weights of the fixed weighted sum; the outputs of ``filter_edges``,
``build_masked_graph`` (its ``edge_index`` / ``edge_attr`` are ``filter_edges``' own, asserted here and stored once) and
``reconstruct_graph`` (node side only, and with edges); the gradients of ``(Wx * x').sum() + (We * edge_attr').sum()`` with
respect to both tokens and the encoder's weight (those with respect to the latent tensors are rows of the integer weights
``Wx[selected]`` / ``We[edges_mask]``: asserted here, not stored); and per
gradient method the eight unweighted losses WITH ``selected_indexes`` = the nodes the selection leaves out, and with the types of
those rows replaced by 9 instead.  Also the table ``k = int((1 - ratio) * n)`` as ``get_masked_indexes`` returns it."""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as MG  # noqa: E402
import make_golden_losses as MGL  # noqa: E402

K_TABLE_N = (1, 7, 20, 100, 1923)
K_TABLE_RATIO = (0.0, 0.15, 0.5, 0.85, 1.0)
F_NODE, F_LATENT, F_EDGE, F_EDGE_LATENT = 5, 6, 3, 4


def make_cases():
    import loss_cases as LC

    cases = {}
    c = MGL.make_cases()["messy"]
    rng = np.random.default_rng(901)
    cases["messy"] = dict(c, selected=rng.permutation(150)[:127].astype(np.int64))
    m = LC.grid2d(7, 9, 300)
    rng = np.random.default_rng(902)
    N, F = 63, 2
    p = m.pos.numpy().astype(np.float64)
    net = rng.standard_normal((N, F)).astype(np.float32)
    ang = np.stack([3.0 * p[:, f % 2] + 2.0 * p[:, (f + 1) % 2] + f for f in range(F)], axis=1)
    sel = np.array([62, 3, 17, 40, 41, 0, 5, 33, 9, 58, 21, 22, 23, 50, 49, 8, 1, 60, 30, 31, 12, 44, 45, 46, 2, 7, 19, 55, 54, 36,
                    37, 14, 27, 26, 61, 10, 48, 16, 35, 6], dtype=np.int64)
    assert len(set(sel.tolist())) == 40
    cases["grid"] = dict(pos=m.pos.numpy(), face=m.face.numpy(), edge_index=m.edge_index.numpy(),
                         node_type=rng.choice([0, 0, 0, 4, 5, 6], size=N).astype(np.float32), F=F, net=net,
                         tgt=(net + rng.standard_normal((N, F))).astype(np.float32),
                         pre=(np.sin(ang) + 0.01 * rng.standard_normal((N, F))).astype(np.float32),
                         std=np.array([0.02, 0.03], dtype=np.float32), mean=np.array([0.01, -0.02], dtype=np.float32), selected=sel)
    for name, c in cases.items():
        rng = np.random.default_rng(910 + len(name))
        N, E = c["pos"].shape[0], c["edge_index"].shape[1]
        c["x"] = rng.standard_normal((N, F_NODE)).astype(np.float32)
        c["edge_attr"] = rng.standard_normal((E, F_EDGE)).astype(np.float32)
        c["node_token"] = rng.standard_normal(F_LATENT).astype(np.float32)
        c["edge_token"] = rng.standard_normal(F_EDGE_LATENT).astype(np.float32)
        c["enc_w"] = rng.standard_normal((F_EDGE_LATENT, F_EDGE)).astype(np.float32)
        c["enc_b"] = rng.standard_normal(F_EDGE_LATENT).astype(np.float32)
        c["full_x"] = rng.standard_normal((N, F_LATENT)).astype(np.float32)   # graph.x of the mesh that is reconstructed
        c["wx"] = rng.integers(-3, 4, size=(N, F_LATENT)).astype(np.float32)
        c["we"] = rng.integers(-3, 4, size=(E, F_EDGE_LATENT)).astype(np.float32)
        c["lat_x"] = rng.standard_normal((len(c["selected"]), F_LATENT)).astype(np.float32)
        c["lat_e_pool"] = rng.standard_normal((E, F_EDGE_LATENT)).astype(np.float32)   # the first E' rows are the latent edge rows
    return cases


def main():
    if not os.path.isdir(MG.REF):
        sys.exit("reference checkout not present: goldens can only be minted in the build container")
    MG.install_standins()
    num_nodes = types.ModuleType("torch_geometric.utils.num_nodes")
    num_nodes.maybe_num_nodes = lambda edge_index, num_nodes=None: int(edge_index.max()) + 1 if num_nodes is None else num_nodes
    utils = types.ModuleType("torch_geometric.utils")
    utils.num_nodes = num_nodes
    sys.modules["torch_geometric.utils"], sys.modules["torch_geometric.utils.num_nodes"] = utils, num_nodes
    for name, attrs in (("meshio", ["Mesh"]), ("torch_geometric.transforms", []), ("torch_geometric.loader", ["ClusterData", "ClusterLoader"])):
        m = types.ModuleType(name)
        for a in attrs:
            setattr(m, a, None)
        sys.modules[name] = m
    torch.manual_seed(0)
    import graphphysics.utils.loss as RL  # noqa: E402
    import graphphysics.utils.meshmask as RM  # noqa: E402
    from graphphysics.utils.nodetype import NodeType as RefNT  # noqa: E402
    from graphphysics.utils.torch_graph import get_masked_indexes as ref_masked_indexes  # noqa: E402
    from torch_geometric.data import Data as _Data  # stand-in

    class Data(_Data):
        def clone(self):
            return Data(**{k: (v.clone() if torch.is_tensor(v) else v) for k, v in self.__dict__.items()})

    RL.device = RM.device = torch.device("cpu")
    masks = [RefNT.NORMAL, RefNT.OUTFLOW]
    out = {}
    t = torch.from_numpy

    for cname, c in make_cases().items():
        N, E = c["pos"].shape[0], c["edge_index"].shape[1]
        sel = t(c["selected"])
        ei = t(c["edge_index"]).long()
        for k in ("pos", "node_type", "net", "tgt", "pre", "std", "mean", "selected", "x", "edge_attr", "node_token", "edge_token",
                  "enc_w", "enc_b", "full_x", "lat_x"):
            out[f"{cname}.{k}"] = c[k]
        out[f"{cname}.wx"], out[f"{cname}.we"] = c["wx"].astype(np.int8), c["we"].astype(np.int8)   # small integers
        out[f"{cname}.face"] = c["face"].astype(np.int16)
        out[f"{cname}.edge_index"] = c["edge_index"].astype(np.int16)

        # filter_edges (the reference sizes its table by edge_index.max() + 1)
        f_ei, f_attr, f_mask = RM.filter_edges(ei, sel, t(c["edge_attr"]))
        out[f"{cname}.filter.edge_index"] = f_ei.numpy().astype(np.int16)
        out[f"{cname}.filter.mask"] = f_mask.numpy()
        assert torch.equal(f_attr, t(c["edge_attr"])[f_mask])   # (the tests rebuild the rows from the mask: not stored twice)
        f_ei2, f_attr2, _ = RM.filter_edges(ei, sel)
        assert f_attr2 is None and torch.equal(f_ei2, f_ei)

        # build_masked_graph
        g = Data(x=t(c["x"]), y=t(c["tgt"]), pos=t(c["pos"]), edge_index=ei.clone(), edge_attr=t(c["edge_attr"]))
        mg, edges_mask = RM.build_masked_graph(g, sel)
        assert mg is g and torch.equal(edges_mask, f_mask) and torch.equal(mg.y, t(c["tgt"]))
        out[f"{cname}.masked.x"], out[f"{cname}.masked.pos"] = mg.x.numpy(), mg.pos.numpy()
        assert torch.equal(mg.edge_index, f_ei) and torch.equal(mg.edge_attr, f_attr)   # stored once, as filter.*
        n_kept = int(edges_mask.sum())
        out[f"{cname}.lat_e"] = c["lat_e_pool"][:n_kept]

        # reconstruct_graph: node side only, then with edges; gradients of the fixed weighted sum
        wx, we = t(c["wx"]), t(c["we"])
        lat_x = t(c["lat_x"]).requires_grad_(True)
        tok = torch.nn.Parameter(t(c["node_token"]).clone())
        full = Data(x=t(c["full_x"]), pos=t(c["pos"]), edge_index=ei.clone())
        rec = RM.reconstruct_graph(full, Data(x=lat_x), sel, tok, edges_mask)
        (wx * rec.x).sum().backward()
        out[f"{cname}.rec_nodes.x"] = rec.x.detach().numpy()
        out[f"{cname}.rec_nodes.d_token"] = tok.grad.numpy()
        assert torch.equal(lat_x.grad, wx[sel])   # (rows of the integer weights: not stored)

        lat_x = t(c["lat_x"]).requires_grad_(True)
        lat_e = t(out[f"{cname}.lat_e"]).requires_grad_(True)
        tok, etok = torch.nn.Parameter(t(c["node_token"]).clone()), torch.nn.Parameter(t(c["edge_token"]).clone())
        enc = torch.nn.Linear(F_EDGE, F_EDGE_LATENT)
        with torch.no_grad():
            enc.weight.copy_(t(c["enc_w"])), enc.bias.copy_(t(c["enc_b"]))
        full = Data(x=t(c["full_x"]), pos=t(c["pos"]), edge_index=ei.clone(), edge_attr=t(c["edge_attr"]))
        rec = RM.reconstruct_graph(full, Data(x=lat_x, edge_attr=lat_e), sel, tok, edges_mask, edge_encoder=enc, edge_mask_token=etok)
        ((wx * rec.x).sum() + (we * rec.edge_attr).sum()).backward()
        out[f"{cname}.rec.x"], out[f"{cname}.rec.edge_attr"] = rec.x.detach().numpy(), rec.edge_attr.detach().numpy()
        assert torch.equal(lat_x.grad, wx[sel]) and torch.equal(lat_e.grad, we[edges_mask])   # rows of the integer weights: not stored
        for k, v in (("d_token", tok.grad), ("d_edge_token", etok.grad), ("d_enc_w", enc.weight.grad)):
            out[f"{cname}.rec.{k}"] = v.numpy()

        # the eight losses with selected_indexes = the nodes the selection leaves out (what a masked-pretraining loss skips is the
        # caller's choice; any index set will do), and with those rows' types replaced by 9
        left_out = torch.from_numpy(np.setdiff1d(np.arange(N), c["selected"]))
        graph = Data(pos=t(c["pos"]), face=t(c["face"]).long(), edge_index=ei)
        node_type, net, tgt, pre, std, mean = (t(c[k]) for k in ("node_type", "net", "tgt", "pre", "std", "mean"))
        u_out, u_tgt = pre + (net * std + mean), pre + (tgt * std + mean)
        type9 = node_type.clone()
        type9[left_out] = 9.0
        out[f"{cname}.left_out"] = left_out.numpy()
        for method in MGL.METHODS:
            with_sel, with_9 = [], []
            for name in MGL.LOSS_ORDER:
                loss = RL.LossType[name].value()
                kw = dict(graph=graph, target=tgt, network_output=net, masks=masks, network_output_physical=u_out,
                          target_physical=u_tgt, gradient_method=method)
                with_sel.append(loss(node_type=node_type, selected_indexes=left_out, **kw))
                with_9.append(loss(node_type=type9, **kw))
            out[f"{cname}.{method}.values_selected"] = torch.stack(with_sel).numpy()
            out[f"{cname}.{method}.values_type9"] = torch.stack(with_9).numpy()

    table = np.zeros((len(K_TABLE_N), len(K_TABLE_RATIO)), dtype=np.int64)
    for i, n in enumerate(K_TABLE_N):
        for j, ratio in enumerate(K_TABLE_RATIO):
            idx = ref_masked_indexes(Data(x=torch.zeros(n, 1)), ratio)
            assert idx.dtype == torch.int64 and len(set(idx.tolist())) == idx.numel()
            table[i, j] = idx.numel()
    out["k_table"], out["k_table.n"], out["k_table.ratio"] = table, np.array(K_TABLE_N), np.array(K_TABLE_RATIO)

    path = os.path.join(HERE, "meshmask.npz")
    np.savez_compressed(path, **out)
    print(f"wrote meshmask.npz  ({os.path.getsize(path) / 1024:.0f} kB, {len(out)} arrays)")


if __name__ == "__main__":
    main()
