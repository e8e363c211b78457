#!/usr/bin/env python3
"""Mint ``simulator_io.npz`` from the REFERENCE implementation (build container only).

Run:  python tests/golden/make_golden_simulator_io.py            (needs the reference checkout)

The reference's ``models/simulator.Simulator`` (with its ``models/layers.Normalizer``) is imported unmodified and run on the CPU
with the stand-ins of make_golden.py (loguru, torch_geometric); the model is ``nn.Identity()``.  The rollout mask is
``build_mask`` of ``training/lightning_module.py:27-35`` restated with the reference's own ``NodeType`` (that module
imports lightning, which is not installed): a float compare.  Only arrays leave this script.

Cases: layouts A, B and E of ``tests/sim_reference.py`` at (N, E) = (9, 7) and (2049, 2047); case A_2049_2047 runs with
``max_accumulations = 2`` on all three normalisers.  Inputs come from ``sim_reference.make_inputs`` (an integer hash:
the tests regenerate them), the file keeps the rows ``sim_reference.sample_rows`` names and the integer column sums of
``8 * [x | y | edge_attr]`` over ALL rows, so that a regenerated input that differs anywhere is noticed.  Per case:
  call 0..2   training:  normalised [node features | target] and edge features (sampled rows), then every buffer of the
              normalisers after the call, packed into one vector;
  call 3      eval:      the same outputs; the buffers are asserted unchanged here;
  post        a hashed network output, ``build_outputs`` of it on the eval inputs, and the same with ``y`` re-imposed where
              the float type is neither NORMAL nor OUTFLOW, on a type column that holds 0.5, -0.5 and 5.5
              (``sim_reference.mask_types``).
``y`` of layout A is 5 columns wide; the reference subtracts whole tensors, so it is handed the first O = 3 columns.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as MG  # noqa: E402
import sim_reference as SR  # noqa: E402

CASES = [(lay, n, e) for lay in ("A", "B", "E") for (n, e) in ((9, 7), (2049, 2047))]
LIMITED = {"A_2049_2047": 2}   # max_accumulations
NET_OUT_CALL, EVAL_CALL = 9, 3
NORMS = ("_node_normalizer", "_output_normalizer", "_edge_normalizer")
BUFFERS = ("_acc_sum", "_acc_sum_squared", "_acc_count", "_num_accumulations")


def main():
    if not os.path.isdir(MG.REF):
        sys.exit("reference checkout not present: goldens can only be minted in the build container")
    MG.install_standins()
    from graphphysics.models.simulator import Simulator as RefSim  # noqa: E402
    from graphphysics.utils.nodetype import NodeType as RefNT  # noqa: E402
    from torch_geometric.data import Data  # stand-in

    t = torch.from_numpy
    cpu = torch.device("cpu")
    out = {}
    for lname, N, E in CASES:
        lay = SR.LAYOUTS[lname]
        case = f"{lname}_{N}_{E}"
        sim = RefSim(model=torch.nn.Identity(), device=cpu, **lay.sim_kwargs())
        limit = LIMITED.get(case)
        if limit is not None:
            for k in NORMS:
                if getattr(sim, k) is not None:
                    getattr(sim, k)._max_accumulations = limit
        out[f"{case}.max_accumulations"] = np.int64(limit if limit is not None else sim._output_normalizer._max_accumulations)
        rn, re = SR.sample_rows(N), SR.sample_rows(E)
        out[f"{case}.rows_n"], out[f"{case}.rows_e"] = rn.astype(np.int32), re.astype(np.int32)

        def snapshot():
            return {k: {b: getattr(getattr(sim, k), b).clone() for b in BUFFERS} for k in NORMS if getattr(sim, k) is not None}

        for c in range(4):
            x, y, ea = SR.make_inputs(lay, N, E, c, SR.case_seed(lname, N))
            i8 = lambda v: np.rint(v.astype(np.float64) * 8).astype(np.int64)   # noqa: E731  (every input is a multiple of 1/8)
            out[f"{case}.c{c}.xy8"] = np.concatenate([i8(x), i8(y)], axis=1)[rn].astype(np.int8)
            out[f"{case}.c{c}.ea8"] = i8(ea)[re].astype(np.int8)
            out[f"{case}.c{c}.colsum8"] = np.concatenate([i8(x).sum(axis=0), i8(y).sum(axis=0), i8(ea).sum(axis=0)])
            ea_t = t(ea)
            batch = Data(x=t(x), y=t(y[:, :lay.O].copy()), pos=torch.zeros(N, 2), edge_attr=ea_t, edge_index=torch.zeros(2, E, dtype=torch.int64))
            training = c != EVAL_CALL
            before = snapshot()
            with torch.no_grad():
                graph, tgt = sim._build_input_graph(batch, training)
            out[f"{case}.c{c}.nodes"] = np.concatenate([graph.x.numpy(), tgt.numpy()], axis=1)[rn]   # [node features | target]
            if lay.edge_w > 0:
                out[f"{case}.c{c}.edges"] = graph.edge_attr.numpy()[re]
            else:
                assert graph.edge_attr is ea_t   # no edge normaliser: the same object passes through
            after = snapshot()
            if not training:
                assert all(torch.equal(before[k][b], after[k][b]) for k in after for b in BUFFERS)
            # per normaliser (node, output, edge if any): [sum (W), sum of squares (W), count, number of accumulations]
            out[f"{case}.c{c}.norm"] = np.concatenate([after[k][b].numpy().reshape(-1) for k in after for b in BUFFERS])
        if limit is not None:   # the third training call left the buffers alone
            assert all(float(after[k]["_num_accumulations"]) == float(limit) for k in after)
            assert np.array_equal(out[f"{case}.c2.norm"], out[f"{case}.c{limit - 1}.norm"])

        net_out = SR.eighths(N, lay.O, 1000 * SR.case_seed(lname, N) + 10 * NET_OUT_CALL)
        with torch.no_grad():
            pred = sim.build_outputs(batch, t(net_out))
        mt = SR.mask_types(x[:, lay.type_idx])
        xm = t(x).clone()
        xm[:, lay.type_idx] = t(mt)
        node_type = xm[:, lay.type_idx]   # build_mask, lightning_module.py:27-35
        mask = torch.logical_not(torch.logical_or(node_type == RefNT.NORMAL, node_type == RefNT.OUTFLOW))
        with torch.no_grad():
            pm = sim.build_outputs(Data(x=xm, y=batch.y), t(net_out))
        pm[mask] = batch.y[mask]
        assert N < 7 or (0 < int(mask.sum()) < N and bool(mask[1]) and bool(mask[3]) and bool(mask[5]))
        # [network output (O) | build_outputs (O) | with the ground truth re-imposed (O) | the type column of the mask (1)]
        out[f"{case}.post"] = np.concatenate([net_out, pred.numpy(), pm.numpy(), mt[:, None]], axis=1)[rn]

    path = os.path.join(HERE, "simulator_io.npz")
    np.savez_compressed(path, **out)
    print(f"wrote simulator_io.npz  ({os.path.getsize(path) / 1024:.0f} kB, {len(out)} arrays)")


if __name__ == "__main__":
    main()
