"""Shared by the masked-mesh tests: the cases of tests/golden/meshmask.npz (minted by tests/golden/make_golden_meshmask.py from
the reference) as arrays, tensors and graphs."""
import os

import numpy as np
import torch

from conftest import GOLDEN

import graph_physics_amd as gp

CASES = ("messy", "grid")
_z = None


def golden():
    global _z
    if _z is None:
        z = np.load(os.path.join(GOLDEN, "meshmask.npz"))
        _z = {k: z[k] for k in z.files}
    return _z


class Case:
    def __init__(self, name):
        z = golden()
        self.name = name
        self.a = {k[len(name) + 1:]: v for k, v in z.items() if k.startswith(name + ".")}
        self.N, self.E = self.a["pos"].shape[0], self.a["edge_index"].shape[1]
        self.edge_index = self.a["edge_index"].astype(np.int64)
        self.mask = self.a["filter.mask"]
        self.kept_attr = self.a["edge_attr"][self.mask]

    def t(self, key, dtype=None):
        v = torch.from_numpy(np.ascontiguousarray(self.a[key]))
        return v if dtype is None else v.to(dtype)

    def graph(self):
        return gp.Graph(x=self.t("x"), y=self.t("tgt"), pos=self.t("pos"), edge_index=torch.from_numpy(self.edge_index),
                        edge_attr=self.t("edge_attr"))

    def encoder(self):
        enc = torch.nn.Linear(3, 4)
        with torch.no_grad():
            enc.weight.copy_(self.t("enc_w")), enc.bias.copy_(self.t("enc_b"))
        return enc
