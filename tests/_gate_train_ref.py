"""References of the fused gate training kernels (include/oeh.h: oeh_gate_apply_fwd / oeh_gate_apply_bwd), CPU only.

`forward64` / `backward64`: a float64 numpy restatement of the header's formulas.  `torch_chain`: the chain the kernels replace as torch
ops on the CPU - the per-head loop of attention.gate_autograd (Linear or Linear-ReLU-Linear on a strided slice per head, stack, sigmoid),
ctx * (gate * s), heads merged, and autograd - in the dtype asked for: float32 on the stored inputs gives err64 (its distance from
float64), float64 checks the restatement.  `make_case`: seeded inputs whose ReLU pre-activations keep clear of zero."""
import numpy as np
import torch

KINK = 1e-3  # no float64 pre-activation of a test input lies this close to zero


def _f64(a):
    return None if a is None else np.asarray(a, dtype=np.float64)


def preact64(hidden, w1, b1, H):
    """u (B,H,T,m) float64 of an MLP predictor: hidden (B,T,H*d), w1 (H,m,d), b1 (H,m)."""
    hidden, w1, b1 = _f64(hidden), _f64(w1), _f64(b1)
    B, T, E = hidden.shape
    x = hidden.reshape(B, T, H, E // H).transpose(0, 2, 1, 3)  # (B,H,T,d)
    return np.einsum("bhtk,hjk->bhtj", x, w1) + b1[None, :, None, :]


def forward64(ctx, hidden, w1, b1, w2, b2, s):
    """(out (B,T,H*d), pi (B,H,T)) in float64: ctx (B,H,T,d), hidden (B,T,H*d), stacked weights (w2, b2 None: Linear predictors)."""
    ctx, hidden, w1, b1, w2, b2 = map(_f64, (ctx, hidden, w1, b1, w2, b2))
    B, H, T, d = ctx.shape
    x = hidden.reshape(B, T, H, d).transpose(0, 2, 1, 3)
    if w2 is None:
        z = np.einsum("bhtk,hk->bht", x, w1) + b1[None, :, None]
    else:
        r = np.maximum(preact64(hidden, w1, b1, H), 0.0)
        z = np.einsum("bhtj,hj->bht", r, w2) + b2[None, :, None]
    pi = 1.0 / (1.0 + np.exp(-z))
    out = (ctx * (pi * s)[..., None]).transpose(0, 2, 1, 3).reshape(B, T, H * d)
    return out, pi


def backward64(dout, ctx, hidden, w1, b1, w2, b2, s):
    """name -> float64 value of dctx (B,H,T,d), dhidden (B,T,H*d), dw1, db1, dw2, db2 (the last two None for Linear predictors)."""
    dout, ctx, hidden, w1, b1, w2, b2 = map(_f64, (dout, ctx, hidden, w1, b1, w2, b2))
    B, H, T, d = ctx.shape
    _, pi = forward64(ctx, hidden, w1, b1, w2, b2, s)
    x = hidden.reshape(B, T, H, d).transpose(0, 2, 1, 3)
    do = dout.reshape(B, T, H, d).transpose(0, 2, 1, 3)
    dctx = do * (pi * s)[..., None]
    dpi = s * (do * ctx).sum(-1)
    dz = dpi * pi * (1.0 - pi)  # (B,H,T)
    if w2 is None:
        dh = dz[..., None] * w1[None, :, None, :]
        res = dict(dw1=np.einsum("bht,bhtk->hk", dz, x), db1=dz.sum((0, 2)), dw2=None, db2=None)
    else:
        u = preact64(hidden, w1, b1, H)
        r = np.maximum(u, 0.0)
        da = np.where(u > 0.0, dz[..., None] * w2[None, :, None, :], 0.0)  # (B,H,T,m)
        dh = np.einsum("bhtj,hjk->bhtk", da, w1)
        res = dict(dw1=np.einsum("bhtj,bhtk->hjk", da, x), db1=da.sum((0, 2)), dw2=np.einsum("bht,bhtj->hj", dz, r), db2=dz.sum((0, 2)))
    res.update(dctx=dctx, dhidden=dh.transpose(0, 2, 1, 3).reshape(B, T, H * d))
    return res


def torch_chain(dout, ctx, hidden, w1, b1, w2, b2, s, dtype=torch.float32):
    """name -> CPU tensor in `dtype`: out, pi and the gradients of the reference chain (gate_autograd's per-head loop, ctx * (gate * s),
    autograd) for the output gradient dout.  Inputs: torch tensors (any device / dtype), upcast exactly."""
    up = lambda t: None if t is None else t.detach().cpu().to(dtype)  # noqa: E731
    dout, ctx, hidden, w1, b1, w2, b2 = map(up, (dout, ctx, hidden, w1, b1, w2, b2))
    B, H, T, d = ctx.shape
    leaves = [t.clone().requires_grad_() for t in (ctx, hidden, w1, b1)] + ([] if w2 is None else [w2.clone().requires_grad_(), b2.clone().requires_grad_()])
    c, hs, W1, B1 = leaves[:4]
    x = hs.view(B, T, H, d).permute(0, 2, 1, 3)
    logits = []
    for h in range(H):
        xh = x[:, h, ...]
        if w2 is None:
            a = torch.nn.functional.linear(xh, W1[h:h + 1], B1[h:h + 1])
        else:
            a = torch.nn.functional.linear(torch.relu(torch.nn.functional.linear(xh, W1[h], B1[h])), leaves[4][h:h + 1], leaves[5][h:h + 1])
        logits.append(a)  # (B,T,1)
    gate = torch.sigmoid(torch.stack(logits, dim=1))  # (B,H,T,1)
    out = (c * (gate * s)).transpose(1, 2).reshape(B, T, H * d)
    (out * dout).sum().backward()
    res = dict(out=out.detach(), pi=gate.detach()[..., 0], dctx=c.grad, dhidden=hs.grad, dw1=W1.grad, db1=B1.grad, dw2=None, db2=None)
    if w2 is not None:
        res.update(dw2=leaves[4].grad, db2=leaves[5].grad)
    return res


def make_case(B, T, H, d, units, dtype, seed, *, scaling=1.25, dead_unit=None, zero_tokens=()):
    """Seeded CPU inputs of one call: dict(ctx (B,H,T,d), hidden (B,T,H*d), dout (B,T,H*d) in `dtype`; w1, b1, w2, b2 fp32 stacked; s).
    The hidden slices of a (token, head) whose float64 pre-activations come within 2 KINK of zero are drawn again until none does (the
    stored, rounded values count).  dead_unit: (h, j) whose b1 is -1e4 (never active).  zero_tokens: (b, t) whose dout row is zero."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *shape: torch.randn(*shape, generator=g)  # noqa: E731
    ctx = rn(B, H, T, d).to(dtype)
    dout = rn(B, T, H * d).to(dtype)
    hidden = rn(B, T, H * d).to(dtype)
    if units == 0:
        w1, b1, w2, b2 = rn(H, d) / d ** 0.5, 0.5 * rn(H), None, None
    else:
        w1, b1, w2, b2 = rn(H, units, d) / d ** 0.5, 0.5 * rn(H, units), rn(H, units) / units ** 0.5, 0.5 * rn(H)
        if dead_unit is not None:
            b1[dead_unit] = -1.0e4
        for _ in range(200):
            u = preact64(hidden.double().numpy(), w1.numpy(), b1.numpy(), H)  # (B,H,T,m)
            near = torch.from_numpy((np.abs(u) < 2 * KINK).any(-1))         # (B,H,T)
            if not near.any():
                break
            fresh = rn(B, T, H * d).to(dtype).view(B, T, H, d)
            hv = hidden.view(B, T, H, d)
            sel = near.permute(0, 2, 1)
            hv[sel] = fresh[sel]
        else:
            raise AssertionError("no draw keeps the pre-activations clear of the ReLU's kink")
    for b, t in zero_tokens:
        dout[b, t] = 0
    return dict(ctx=ctx, hidden=hidden, dout=dout, w1=w1, b1=b1, w2=w2, b2=b2, s=scaling)


def kink_clear(case, H):
    """The precondition of the float64 comparison: in float64 no pre-activation of the case lies within KINK of zero."""
    if case["w2"] is None:
        return True
    u = preact64(case["hidden"].detach().cpu().double().numpy(), case["w1"].cpu().numpy(), case["b1"].cpu().numpy(), H)
    return bool((np.abs(u) >= KINK).all())
