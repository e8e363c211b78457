"""Shared by the loss tests: the cases of tests/golden/physics_losses.npz (minted by tests/golden/make_golden_losses.py from the
reference) as graphs and tensors on a device."""
import os

import numpy as np
import torch

from conftest import GOLDEN

import graph_physics_amd as gp

CASES = ("cyl", "cyl_moved", "tet", "surf", "messy")
METHODS = ("finite_diff", "least_squares")
LOSS_ORDER = ("L2LOSS", "COSINEL2LOSS", "L1SMOOTHLOSS", "GRADIENTL2LOSS", "CONVECTIONL2LOSS", "DIVERGENCEL2LOSS", "DIVERGENCEL1LOSS",
              "DIVERGENCEL1SMOOTHLOSS")
SECTIONS = {
    "pinn": {"type": ["l2loss", "gradientl2loss", "divergencel2loss"], "weights": [0.5, 0.5, 0.5], "gradient_method": "finite_diff"},
    "panels": {"type": ["l2loss", "gradientl2loss", "convectionl2loss", "divergencel1loss"], "weights": [1, 1e-2, 1e-4, 1e-1],
               "gradient_method": "least_squares"},
}
MASKS = (gp.NodeType.NORMAL, gp.NodeType.OUTFLOW)

_z = None


def fixture():
    global _z
    if _z is None:
        z = np.load(os.path.join(GOLDEN, "physics_losses.npz"))
        _z = {k: z[k] for k in z.files}
    return _z


class Case:
    """one fixture case on ``device``: ``graph`` (pos, face, edge_index), the normalised ``net`` / ``tgt``, ``node_type`` and the
    affine map to the physical fields (``physical``)"""

    def __init__(self, name, device):
        z = fixture()
        base = "cyl" if name == "cyl_moved" else name   # cyl_moved stores only its positions
        t = lambda k, src=base: torch.from_numpy(z[f"{src}.{k}"]).to(device)  # noqa: E731
        self.name = name
        self.graph = gp.Graph(pos=t("pos", name), face=t("face").long(), edge_index=t("edge_index").long())
        self.net, self.tgt, self.node_type = t("net"), t("tgt"), t("node_type")
        self.pre, self.std, self.mean = t("pre"), t("std"), t("mean")

    def physical(self, x):
        return self.pre + (x * self.std + self.mean)

    def ref(self, key):
        return torch.from_numpy(np.asarray(fixture()[f"{self.name}.{key}"]))

    def dnet64(self, method, sec):
        return self.ref(f"{method}.{sec}.dnet").double() + self.ref(f"{method}.{sec}.dnet64_minus32").double()

    def grad_bar(self, method, sec):
        """max(1e-5, the fp32 reference's own recorded distance from fp64)"""
        return max(1e-5, float(self.ref(f"{method}.{sec}.dnet_ref_dist")))


def single_loss(c, name, method):
    """one loss type alone, called with the reference's keyword set"""
    loss = gp.LossType[name].value()
    return loss(graph=c.graph, target=c.tgt, network_output=c.net, node_type=c.node_type, masks=list(MASKS),
                network_output_physical=c.physical(c.net), target_physical=c.physical(c.tgt), gradient_method=method)


def section_loss(c, sec, method):
    """a shipped ``loss`` section evaluated with ``method``: (total, weighted terms, d total / d net)"""
    loss, _ = gp.get_loss({"loss": dict(SECTIONS[sec], gradient_method=method)})
    net = c.net.clone().requires_grad_(True)
    total, terms = loss(graph=c.graph, target=c.tgt, network_output=net, node_type=c.node_type, masks=list(MASKS),
                        network_output_physical=c.physical(net), target_physical=c.physical(c.tgt), gradient_method=method,
                        return_all_losses=True)
    total.backward()
    return total.detach(), torch.stack([t.detach() for t in terms]), net.grad
