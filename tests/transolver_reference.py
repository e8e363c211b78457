"""fp64 restatement of the Transolver physics attention in the project's own words (what tests/test_hip_transolver.py holds the kernels
of include/mgn_hip_slice.h to, and tests/test_transolver_host.py the golden arrays).

It takes the fp32 uniforms ``u`` and forms the Gumbel noise ``g = -log(-log(u + 1e-8) + 1e-8)`` IN FP32, exactly as stated, before
widening: in fp64 ``u + 1e-8`` does not round away, and ``g`` would differ by about 0.16 for ``u`` next to 1."""
import math

import numpy as np
import torch

CLAMP = 0.01


def gumbel32(u: torch.Tensor) -> torch.Tensor:
    u = u.detach().float().cpu()
    return (-torch.log(-torch.log(u + 1e-8) + 1e-8)).double()


def gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def weights(xm, Ws, bs, W1, b1, w2, b2, bias, u):
    """(w [N, H, G], t2 [N, H], tpre [N, H]) from x_mid [N, H, C]; all fp64 but the noise"""
    h1 = gelu(torch.einsum("nhc,gc->nhg", xm, W1) + b1)
    t2 = torch.einsum("nhg,g->nh", h1, w2.reshape(-1)) + b2.reshape(())
    tpre = gelu(t2) + bias.reshape(1, -1)
    t = torch.clamp(tpre, min=CLAMP)
    a = torch.einsum("nhc,gc->nhg", xm, Ws) + bs
    return torch.softmax((a + gumbel32(u)) / t.unsqueeze(-1), dim=-1), t2, tpre


def aggregate(w, x):
    """(S [H, G, C], norm [H, G])"""
    return torch.einsum("nhg,nhc->hgc", w, x), w.sum(0)


def expand(w, tok):
    return torch.einsum("nhg,hgc->nhc", w, tok)


def tokens(S, norm, Wq, Wk, Wv, gate=None):
    """the token part: token = S / (norm + 1e-5), attention among the G tokens of a head at scale C^-0.5; with ``gate`` = (W0, b0, W2, b2)
    the result is multiplied by sigmoid(W2 silu(W0 cat(token, out) + b0) + b2)"""
    token = S / (norm + 1e-5).unsqueeze(-1)
    q, k, v = token @ Wq.t(), token @ Wk.t(), token @ Wv.t()
    out = torch.softmax(q @ k.transpose(1, 2) / math.sqrt(S.shape[-1]), dim=-1) @ v
    if gate is not None:
        W0, b0, W2, b2 = gate
        h = torch.cat([token, out], dim=-1) @ W0.t() + b0
        out = torch.sigmoid((h * torch.sigmoid(h)) @ W2.t() + b2) * out
    return out


def load_golden():
    """tests/golden/transolver.npz: numeric arrays as tensors, name lists as numpy arrays of strings"""
    import os
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "transolver.npz"))
    return {k: (torch.from_numpy(z[k]) if z[k].dtype.kind in "fiu" else z[k]) for k in z.files}


def unpack_case(Z, name):
    """the arrays of one case of tests/golden/transolver.npz: (meta dict, tensors dict, state dict, fp64 gradients dict, fp32-run errors dict)"""
    pre = name + "."
    m = [int(v) for v in Z[pre + "meta"]]
    meta = dict(N=m[0], hidden=m[1], heads=m[2], G=m[3], blocks=m[4], n_in=m[5], n_out=m[6], rope=m[7], gate=bool(m[8]), temporal=bool(m[9]), ref=m[10])
    keys = [str(k) for k in np.asarray(Z[pre + "keys"])]
    shapes = {k: [int(v) for v in s if int(v) > 0] for k, s in zip(keys, np.asarray(Z[pre + "shapes"]))}
    flat, at, state = Z[pre + "w"], 0, {}
    for k in keys:
        n = int(np.prod(shapes[k])) if shapes[k] else 1
        state[k] = flat[at:at + n].reshape(shapes[k]).clone()
        at += n
    gkeys = [str(k) for k in np.asarray(Z[pre + "gkeys"])]
    flat, at, g64 = Z[pre + "f64.g.w"], 0, {}
    for k in gkeys:
        n = int(np.prod(shapes[k])) if shapes[k] else 1
        g64[k] = flat[at:at + n].reshape(shapes[k]).clone()
        at += n
    err = {k: float(e) for k, e in zip(gkeys, Z[pre + "f32err.g.w"])}
    err["out"], err["g.x"] = float(Z[pre + "f32err.out"]), float(Z[pre + "f32err.g.x"])
    T = {k: Z[pre + k] for k in ("x", "pos", "dy", "u", "tpre", "f64.out", "f64.g.x", "f32.out", "f32.g.x")}
    return meta, T, state, g64, err


def bound(conv: float, ref_err: float) -> float:
    """the bound of one compared tensor: the project's convention (1e-5 of the fp64 tensor's largest entry forward, 2e-5 for gradients) or
    4 x the reference's own fp32-against-fp64 error for that tensor, whichever is larger (the factor covers the last bits of another
    expf / logf / erff and another summation order over the nodes)"""
    return max(conv, 4.0 * ref_err)
