"""Tensor-level entry points over the C ABI (include/oeh.h).  torch is plumbing here: device memory,
the current HIP stream, dtype/stride bookkeeping.  Every function launches HIP kernels from
liboeh_hip.so; tensors that are not on a GPU are an error (there is no CPU path in this package).
"""
from __future__ import annotations

import ctypes as C
import functools
import threading
from dataclasses import dataclass
from typing import Optional

import torch

from . import _lib
from ._lib import OEH_BF16, OEH_F16, OEH_F32, oeh_attn_desc, oeh_attn_opts, oeh_dropout, oeh_fq, oeh_fq_desc

_DT = {torch.float16: OEH_F16, torch.bfloat16: OEH_BF16, torch.float32: OEH_F32}


@dataclass(frozen=True)
class SoftmaxSpec:
    """One entry of the reference's --attn_softmax registry (models/softmax.py:22-64):
    base 0 = torch softmax, 1 = softmax_1; clip -> clip(p*(eta-gamma)+gamma, 0, 1)."""

    base: int = 1
    clip: bool = False
    gamma: float = 0.0
    eta: float = 1.0


@dataclass
class FakeQuantSpec:
    """Fixed-range asymmetric quantiser grid (uniform_quantizers.py:72-82): fp32 scale, integer zero point, qmax."""

    scale: float
    zero_point: float
    qmax: float = 255.0
    dump: Optional[torch.Tensor] = None  # uint8 tensor receiving the indices (tests)

    @staticmethod
    def from_delta(delta: float, zero_float: float, n_bits: int = 8, eps: float = 1e-8, dump=None) -> "FakeQuantSpec":
        import numpy as np

        qmax = float(2.0 ** n_bits - 1)
        scale = float(np.float32(max(float(delta), eps)))
        zp = float(min(max(float(np.rint(np.float64(zero_float))), 0.0), qmax))
        return FakeQuantSpec(scale, zp, qmax, dump)


@dataclass
class AttnFakeQuant:
    scores: Optional[FakeQuantSpec] = None
    probs: Optional[FakeQuantSpec] = None
    ctx: Optional[FakeQuantSpec] = None
    ctx_before_gate: bool = True  # OPT order; False = BERT order (quantise after the gate)
    ctx_emit_index: bool = False  # the output holds the context quantiser's integers idx - zp (include/oeh.h: ctx_emit_index)


def grad_recording(*ts) -> bool:
    """True when autograd is recording and one of the tensors is part of the graph: the callers then take the differentiable
    torch-op form of the same op chain (attention.unfused_core, softmax.softmax_autograd, attention.gate_autograd) - on the GPU, like
    everything else here - instead of the forward-only HIP kernels."""
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in ts)


def _need_gpu(*ts, allow_grad: bool = False):
    """Every tensor on ONE GPU, and (unless `allow_grad`: the torch-op path) none of them part of an autograd graph being
    recorded: the library is the only implementation (no CPU path) and it is forward-only - its outputs carry no grad_fn, so
    running it under autograd would drop the gradients of q / k / v / gate silently.  The modules route such calls to the torch-op
    path before they get here (`grad_recording`); a direct op call raises (inference: `with torch.no_grad():`)."""
    dev = None
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise _lib.OehError("outeffhop_amd ops need GPU tensors: the HIP library is the only implementation")
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise _lib.OehError(f"outeffhop_amd ops need all tensors on one GPU, got {dev} and {t.device}")
    if not allow_grad and grad_recording(*ts):
        raise _lib.OehError("outeffhop_amd is forward-only (the backward pass is out of scope, DESIGN.md section 7): an input requires "
                            "grad while autograd is recording - run inference under torch.no_grad() / torch.inference_mode()")
    return dev


class _on_device:
    """Make the tensors' GPU the current HIP device for the launch (kernels run on the stream of the CURRENT device)."""

    def __init__(self, dev):
        self.dev, self.prev = dev, None

    def __enter__(self):
        if self.dev is not None and self.dev.index is not None and self.dev.index != torch.cuda.current_device():
            self.prev = torch.cuda.current_device()
            torch.cuda.set_device(self.dev)

    def __exit__(self, *exc):
        if self.prev is not None:
            torch.cuda.set_device(self.prev)


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)  # the handle without building a Stream object (9 us -> 0.5 us)


def _stream() -> C.c_void_p:
    if _raw_stream is not None:
        return C.c_void_p(_raw_stream(torch.cuda.current_device()))
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t: Optional[torch.Tensor]) -> C.c_void_p:
    return C.c_void_p(0 if t is None else t.data_ptr())


def _fill_fq(dst: oeh_fq, spec: Optional[FakeQuantSpec]):
    if spec is None:
        dst.enable = 0
        return
    dst.enable = 1
    dst.scale, dst.zero_point, dst.qmax = spec.scale, spec.zero_point, spec.qmax
    if spec.dump is not None:
        assert spec.dump.dtype == torch.uint8 and spec.dump.is_contiguous() and spec.dump.is_cuda
        dst.dump_idx = spec.dump.data_ptr()


# ---- host marshalling shared by the entry points: argument checks, the descriptors of include/oeh.h, the per-stream scratch
def _need_dtype(x: torch.Tensor) -> None:
    if x.dtype not in _DT:
        raise ValueError(f"unsupported dtype {x.dtype}")


def _need_f64(t: torch.Tensor, n: int, message: str) -> None:
    """A device-side float64 vector of the C ABI (a range, a running state, a meter, the losses): n contiguous elements."""
    if t.dtype != torch.float64 or t.numel() != n or not t.is_contiguous():
        raise ValueError(message)


def _check_qkv(q, k, v):
    """q (B,H,Sq,D), k and v (B,H,Sk,D) in one of the storage dtypes; an input whose head-dim stride is not 1 comes back as a contiguous
    copy (the kernels read contiguous head dims)."""
    if q.dim() != 4 or k.dim() != 4 or v.dim() != 4:
        raise ValueError("q, k, v must be 4-D (B,H,S,D) views")
    B, H, Sq, D = q.shape
    Sk = k.shape[2]
    if k.shape != (B, H, Sk, D) or v.shape != (B, H, Sk, D):
        raise ValueError(f"shape mismatch: q {tuple(q.shape)} k {tuple(k.shape)} v {tuple(v.shape)}")
    if not (q.dtype == k.dtype == v.dtype) or q.dtype not in _DT:
        raise ValueError(f"q/k/v dtypes must match and be fp16/bf16/fp32, got {q.dtype}, {k.dtype}, {v.dtype}")
    fix = lambda t: t if t.stride(3) == 1 else t.contiguous()  # noqa: E731
    return fix(q), fix(k), fix(v)


def _attn_desc(q, k, v, o, dtype: int, o_dtype: int, softmax: SoftmaxSpec, scale, scale_div, causal, clamp_min, mask_min: Optional[float],
               scores_dtype: torch.dtype) -> oeh_attn_desc:
    """The part of an `oeh_attn_desc` every launching entry point fills: the geometry of q (B,H,Sq,D) against Sk keys, the storage and output
    dtype codes, the (batch, head, row) strides of the four tensors, scale, softmax, causal / clamp_min / mask_min.  mask_min None: finfo.min
    of `scores_dtype`, the dtype the reference would hold the scores in (include/oeh.h).  Masks and gate: `_set_key_pad`, `_set_full_mask`,
    `_set_gate`."""
    d = oeh_attn_desc()
    d.B, d.H, d.Sq, d.D = q.shape
    d.Sk = k.shape[2]
    d.dtype, d.o_dtype = dtype, o_dtype
    for name, t in (("q_stride", q), ("k_stride", k), ("v_stride", v), ("o_stride", o)):
        getattr(d, name)[:] = [t.stride(0), t.stride(1), t.stride(2)]
    d.scale, d.scale_div = float(scale), float(scale_div)
    d.softmax_base, d.clip, d.gamma, d.eta = int(softmax.base), int(bool(softmax.clip)), float(softmax.gamma), float(softmax.eta)
    d.causal, d.clamp_min = int(bool(causal)), int(bool(clamp_min))
    d.mask_min = float(torch.finfo(scores_dtype).min if mask_min is None else mask_min)
    return d


def _probe_desc(B, H, Sq, Sk, D, dtype, *, scale=1.0, scale_div=0.0, base=1, clip=False, gamma=-0.025, causal=False, mask_min=None) -> oeh_attn_desc:
    """The host-only descriptor of the `*_variant` probes: what decides the kernel, without tensors - no strides, no o_dtype, and of a
    pointer only its nullness matters (nothing is dereferenced: the callers set 1 for "present").  Clipping as the registry has it (eta 1)."""
    d = oeh_attn_desc()
    d.B, d.H, d.Sq, d.Sk, d.D, d.dtype = B, H, Sq, Sk, D, _DT[dtype]
    d.scale, d.scale_div = float(scale), float(scale_div)
    d.softmax_base, d.causal = int(base), int(bool(causal))
    d.mask_min = float(torch.finfo(torch.float32).min if mask_min is None else mask_min)  # (no tensor to take the default's dtype from)
    if clip:
        d.clip, d.gamma, d.eta = 1, float(gamma), 1.0
    return d


def _set_key_pad(d: oeh_attn_desc, keep: list, mask: torch.Tensor, i8: bool = False) -> None:
    """The additive key-padding vector as the kernel reads it: fp16 / fp32, (B,Sk) with contiguous keys (anything else is converted to
    fp32).  `i8`, the INT8-storage path: a mask of ONE row serves every batch through a zero batch stride, and rows that are a stride
    apart are read in place; the other paths always hand over a dense (B,Sk) copy.  `key_pad_boolean` is the caller's to set."""
    B, Sk = d.B, d.Sk
    if i8:
        m = mask if mask.dtype in (torch.float16, torch.float32) else mask.float()
        m = m.reshape(B, Sk) if m.numel() == B * Sk else m.reshape(1, Sk).expand(B, Sk)
        if m.stride(1) != 1:
            m = m.contiguous()
    else:
        m = mask.reshape(B, Sk)
        if m.dtype not in (torch.float16, torch.float32):
            m = m.float()
        m = m.contiguous()
    keep.append(m)
    d.key_pad_mask, d.key_pad_dtype, d.key_pad_stride = m.data_ptr(), _DT[m.dtype], m.stride(0)


def _set_full_mask(d: oeh_attn_desc, keep: list, full_mask: torch.Tensor) -> None:
    """The additive (B,1,Sq,Sk) mask: fp16 / fp32 with contiguous keys, read in place where it already is."""
    B, Sq, Sk = d.B, d.Sq, d.Sk
    if full_mask.shape != (B, 1, Sq, Sk):
        raise ValueError(f"Attention mask should be of size {(B, 1, Sq, Sk)}, but is {tuple(full_mask.shape)}")
    m = full_mask if full_mask.dtype in (torch.float16, torch.float32) else full_mask.float()
    m = m if m.stride(3) == 1 else m.contiguous()
    keep.append(m)
    d.full_mask, d.full_mask_dtype = m.data_ptr(), _DT[m.dtype]
    d.full_mask_stride[:] = [m.stride(0), m.stride(2)]


def _set_gate(d: oeh_attn_desc, keep: list, gate: torch.Tensor) -> None:
    """Gate values, fp32, broadcast to (B,H,Sq,1) by zero strides."""
    g = gate.to(torch.float32)
    while g.dim() < 4:
        g = g.unsqueeze(0)
    g = g.expand(d.B, d.H, d.Sq, 1)
    keep.append(g)
    d.gate = g.data_ptr()
    d.gate_stride[:] = [g.stride(0), g.stride(1), g.stride(2)]


def _fq_desc(fq: Optional[AttnFakeQuant], always: bool = False) -> Optional[oeh_fq_desc]:
    """The `oeh_fq_desc` of `fq`; None when no quantiser is enabled (the entry points then run their forms without quantisers), unless
    `always`."""
    if not always and (fq is None or not (fq.scores or fq.probs or fq.ctx)):
        return None
    fqd = oeh_fq_desc()
    _fill_fq(fqd.scores, fq.scores)
    _fill_fq(fqd.probs, fq.probs)
    _fill_fq(fqd.ctx, fq.ctx)
    fqd.ctx_quant_before_gate = int(bool(fq.ctx_before_gate))
    fqd.ctx_emit_index = int(bool(fq.ctx_emit_index))
    return fqd


# what the `*_variant` probes ask about with fq=True: scores and probabilities on full 8-bit grids of scale 1 (every other field zero)
_PROBE_FQ = AttnFakeQuant(FakeQuantSpec(1.0, 0.0), FakeQuantSpec(1.0, 0.0), ctx_before_gate=False)


def _scratch(table: dict, dev, nbytes: int) -> torch.Tensor:
    """The current stream's work buffer of one entry point on `dev`, from that entry point's `table`: (device index, stream handle) ->
    buffer, grown to the largest request so far.  Per stream, because two calls on different streams of one GPU may run at the same time
    and must not share partial results.  Bounded, because streams come and go (a recycled handle simply reuses its buffer): at 32 entries
    the table starts over instead of keeping one buffer per stream ever seen.  Under graph capture the call gets a buffer of its own
    instead, allocated inside the capture: it then lives in the graph's private pool for as long as the graph does - a cached buffer may
    be replaced (a larger request, the table starting over) and freed while a graph that recorded its address is still replayed."""
    with _on_device(dev):
        if torch.cuda.is_current_stream_capturing():
            return torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=dev)
        key = (dev.index, torch.cuda.current_stream().cuda_stream)
    work = table.get(key)
    if work is None or work.numel() * 8 < nbytes:
        if len(table) >= 32:
            table.clear()  # (buffers still referenced by enqueued work stay alive in the caching allocator's stream order)
        work = table[key] = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=dev)
    return work


def attn_fwd(
    q: torch.Tensor,
    k: torch.Tensor,
    v: torch.Tensor,
    *,
    softmax: SoftmaxSpec = SoftmaxSpec(),
    scale: float = 1.0,
    scale_div: float = 0.0,
    key_pad_mask: Optional[torch.Tensor] = None,
    full_mask: Optional[torch.Tensor] = None,
    key_pad_boolean: bool = False,
    causal: bool = False,
    clamp_min: bool = False,
    mask_min: Optional[float] = None,
    gate: Optional[torch.Tensor] = None,
    fq: Optional[AttnFakeQuant] = None,
    out: Optional[torch.Tensor] = None,
    gate_mlp: Optional["GatePredictor"] = None,
    out_dtype: Optional[torch.dtype] = None,
    pv_pairs: bool = False,
    _prepared: Optional[list] = None,
) -> torch.Tensor:
    """Fused attention core.  q,k,v are logical (B,H,S,D) views (any batch/head/seq strides, unit head-dim
    stride).  Returns the logical (B,H,Sq,D) result, stored (B,Sq,H,D)-contiguous unless `out` is given, so the
    reference's head merge (bert_attention.py:335-337) is a free `.permute(0,2,1,3).reshape(B,Sq,H*D)`.

    key_pad_mask: additive (B,Sk) [or anything reshapeable to it, e.g. HF's (B,1,1,Sk)]; key_pad_boolean: the caller's promise that
    its entries are 0 or <= -1e4 only (include/oeh.h - lets the fused INT8 chain stay on the quantiser grid with padded keys);
    full_mask: additive (B,1,Sq,Sk); gate: fp32, broadcastable to (B,H,Sq,1), already times the scaling factor.
    out_dtype=torch.float32 with fp16 / bf16 inputs: the output straight from the kernel's fp32 accumulators (include/oeh.h: o_dtype) -
    the kernel's arithmetic before the output rounding, which is how tests / smoke / bench check the "within 1e-3" contract on the
    kernel that ships; the one-pass and full-row kernels only (OehError -95 otherwise).
    pv_pairs=True (fp32 storage): the context to fp32 accuracy too - the probability operand of the second product as an fp16 pair
    (include/oeh.h: oeh_attn_opts); OehError -95 with 16-bit storage, fake-quant or `gate_mlp`."""
    # ---- the repeated call (round 5): same geometry and options as an earlier call -> that call's prebuilt descriptor, pointers patched.
    # The Python below this block is ~13 us per call (checks, a 40-field ctypes descriptor, mask / gate views) against ~3 us for the launch of a
    # prebuilt one, and the fp16 BERT-base layer is host-bound in eager mode.  Only the plain forms (no fused quantisers, no in-kernel gate predictor,
    # no (B,1,Sq,Sk) mask, no caller's `out`, inference).
    fkey = None
    if (FAST_CALLS and out is None and gate_mlp is None and fq is None and full_mask is None and _prepared is None and out_dtype is None
            and q.is_cuda and q.dim() == 4 and q.device.index == torch.cuda.current_device()
            and not (torch.is_grad_enabled() and (q.requires_grad or k.requires_grad or v.requires_grad or (gate is not None and gate.requires_grad)))):
        fkey = _fast_key(q, k, v, softmax, scale, scale_div, key_pad_mask, key_pad_boolean, causal, clamp_min, mask_min, gate)
        if fkey is not None and pv_pairs:
            fkey = ("pv_pairs", fkey)
        hit = _fast_tls.table.get(fkey) if fkey is not None else None
        if hit is not None:
            fn, d, oshape, odt = hit
            o = torch.empty(oshape, dtype=odt, device=q.device).permute(0, 2, 1, 3)
            if key_pad_mask is not None:
                d.key_pad_mask = key_pad_mask.data_ptr()
            if gate is not None:
                d.gate = gate.data_ptr()
            rc = fn(C.byref(d), C.c_void_p(q.data_ptr()), C.c_void_p(k.data_ptr()), C.c_void_p(v.data_ptr()), C.c_void_p(o.data_ptr()), None, _stream())
            if rc != 0:
                _lib.check(rc, "oeh_attn_fwd")
            return o
    dev = _need_gpu(q, k, v, key_pad_mask, full_mask, gate, out)
    q, k, v = _check_qkv(q, k, v)
    B, H, Sq, D = q.shape
    Sk = k.shape[2]
    odt = q.dtype if out_dtype is None else out_dtype
    if odt != q.dtype and not (odt == torch.float32 and q.dtype in (torch.float16, torch.bfloat16)):
        raise ValueError(f"out_dtype must be the input dtype, or float32 for fp16 / bf16 inputs (got {odt} for {q.dtype})")
    Dp = _matrix_core_head_dim(D, Sq, Sk, plain=key_pad_mask is None and full_mask is None and not causal and fq is None)
    if (Dp != D and gate_mlp is None and _prepared is None and odt == q.dtype and (out is None or out.shape == (B, H, Sq, D))
            and not (fq is not None and fq.ctx is not None and fq.ctx.dump is not None)):
        # A head dim between the matrix-core kernels' (OPT-2.7b / ViT-H: 80; 96; 48; 16 with long rows ...): zero columns change
        # neither the scores nor the other columns of the product - three pad copies and the next kernel size up instead of the
        # any-shape kernel (one workgroup per query row, ~100x slower)
        pad = lambda t: torch.nn.functional.pad(t, (0, Dp - D))  # noqa: E731
        res = attn_fwd(pad(q), pad(k), pad(v), softmax=softmax, scale=scale, scale_div=scale_div, key_pad_mask=key_pad_mask, full_mask=full_mask,
                       key_pad_boolean=key_pad_boolean, causal=causal, clamp_min=clamp_min, mask_min=float(torch.finfo(q.dtype).min if mask_min is None else mask_min), gate=gate,
                       fq=fq, pv_pairs=pv_pairs)[..., :D]
        if out is None:
            return res
        out.copy_(res)
        return out
    if out is None:
        out = torch.empty((B, Sq, H, D), dtype=odt, device=q.device).permute(0, 2, 1, 3)
    elif out.shape != (B, H, Sq, D) or out.dtype != odt or out.stride(3) != 1:
        raise ValueError("out must be a (B,H,Sq,D) view with unit head-dim stride and the input dtype (or out_dtype)")

    # o_dtype: the dtype of `out` (read for 16-bit inputs only when it says OEH_F32)
    d = _attn_desc(q, k, v, out, _DT[q.dtype], _DT[odt], softmax, scale, scale_div, causal, clamp_min, mask_min, q.dtype)
    keep = []
    if key_pad_mask is not None:
        _set_key_pad(d, keep, key_pad_mask)
        d.key_pad_boolean = int(bool(key_pad_boolean))  # the caller's promise (include/oeh.h): this entry point alone passes it on
    if full_mask is not None:
        _set_full_mask(d, keep, full_mask)
    if gate is not None:
        _set_gate(d, keep, gate)
    if gate_mlp is not None:
        if gate is not None:
            raise ValueError("pass either `gate` (values) or `gate_mlp` (predictor evaluated in the kernel), not both")
        gm = gate_mlp
        hid = gm.hidden
        _need_gpu(hid, gm.w1, gm.b1, gm.w2, gm.b2, gm.out)
        if hid.shape != (B, Sq, H * D) or hid.dtype != q.dtype or hid.stride(2) != 1:
            raise ValueError(f"gate_mlp.hidden must be (B,Sq,H*D) = {(B, Sq, H * D)} in the dtype of q with a contiguous last dim")
        f32c = lambda t: None if t is None else t.detach().to(torch.float32).contiguous()  # noqa: E731
        w1, b1, w2, b2 = f32c(gm.w1), f32c(gm.b1), f32c(gm.w2), f32c(gm.b2)
        keep.extend([hid, w1, b1, w2, b2, gm.out])
        d.gate_hidden = hid.data_ptr()
        d.gate_hidden_stride[:] = [hid.stride(0), hid.stride(1)]
        d.gate_w1, d.gate_b1 = w1.data_ptr(), b1.data_ptr()
        d.gate_units = 0 if w1.dim() == 2 else w1.shape[1]
        if d.gate_units > 0:
            d.gate_w2, d.gate_b2 = w2.data_ptr(), b2.data_ptr()
        d.gate_scaling = float(gm.scaling)
        if gm.out is not None:
            if gm.out.shape != (B, H, Sq) or gm.out.dtype != torch.float32 or not gm.out.is_contiguous():
                raise ValueError("gate_mlp.out must be a contiguous fp32 (B,H,Sq) tensor")
            d.gate_out = gm.out.data_ptr()
    fqd = _fq_desc(fq)
    lib = _lib.load()
    fn, what = lib.oeh_attn_fwd, "oeh_attn_fwd"
    if pv_pairs:  # oeh_attn_fwd_ex with the options bound: the same call signature as oeh_attn_fwd from here on
        opts = oeh_attn_opts(pv_pairs=1)
        keep.append(opts)
        fn, what = functools.partial(_attn_fwd_ex, lib, C.byref(opts)), "oeh_attn_fwd_ex"
    if _prepared is not None:  # hand back the prebuilt C call instead of launching (bench / hipGraph loops)
        _warn_if_any_shape_kernel(lib, d, fqd, softmax)
        args = (C.byref(d), _ptr(q), _ptr(k), _ptr(v), _ptr(out), None if fqd is None else C.byref(fqd))
        _prepared.extend([fn, args, (d, fqd, keep, q, k, v, out)])
        return out
    with _on_device(dev):
        rc = fn(C.byref(d), _ptr(q), _ptr(k), _ptr(v), _ptr(out), None if fqd is None else C.byref(fqd), _stream())
    _lib.check(rc, what)
    _warn_if_any_shape_kernel(lib, d, fqd, softmax)  # (after the launch: a call the library refuses raises above and has run nothing)
    if fkey is not None and fqd is None and q.stride(3) == 1 and k.stride(3) == 1 and v.stride(3) == 1 and out.shape == (B, H, Sq, D):
        # remember the descriptor for the next call of this geometry (its mask / gate pointers are patched per call; the views `keep` holds
        # were only needed for THIS call's pointers)
        if len(_fast_tls.table) >= 256:
            _fast_tls.table.clear()
        _fast_tls.table[fkey] = (fn, d, (B, Sq, H, D), odt)
    return out


def _attn_fwd_ex(lib, opts, d, q, k, v, o, fqd, stream):
    return lib.oeh_attn_fwd_ex(d, opts, q, k, v, o, fqd, stream)


FAST_CALLS = True


class _FastCalls(threading.local):
    """geometry + options -> (C function, descriptor, output shape, output dtype): see attn_fwd.  Per THREAD: a cached descriptor's mask / gate
    pointers are patched right before the call, and ctypes releases the GIL inside it."""

    def __init__(self):
        self.table = {}


_fast_tls = _FastCalls()


def _fast_key(q, k, v, softmax, scale, scale_div, key_pad_mask, key_pad_boolean, causal, clamp_min, mask_min, gate):
    """What a prebuilt `oeh_attn_desc` depends on besides the four data pointers and the mask / gate pointers; None: not a plain call."""
    if k.dim() != 4 or v.dim() != 4 or k.device != q.device or v.device != q.device or not (q.dtype == k.dtype == v.dtype):
        return None
    if q.stride(3) != 1 or k.stride(3) != 1 or v.stride(3) != 1 or q.shape[3] not in (32, 64, 128):
        return None
    pk = None
    if key_pad_mask is not None:
        # (the vector as the slow path would hand it over unchanged: (B, Sk), fp16 / fp32, contiguous rows, on the same GPU)
        if (key_pad_mask.dim() != 2 or key_pad_mask.dtype not in (torch.float16, torch.float32) or key_pad_mask.stride(1) != 1 or key_pad_mask.stride(0) != key_pad_mask.shape[1]
                or key_pad_mask.device != q.device or key_pad_mask.shape != (q.shape[0], k.shape[2])):
            return None
        pk = key_pad_mask.dtype
    gk = None
    if gate is not None:
        if gate.dim() != 4 or gate.dtype != torch.float32 or gate.device != q.device:
            return None
        gk = (gate.shape, gate.stride())
    return (q.shape, q.stride(), k.shape, k.stride(), v.shape, v.stride(), q.dtype, q.device, softmax, float(scale), float(scale_div), pk, bool(key_pad_boolean), bool(causal),
            bool(clamp_min), mask_min, gk)


def _matrix_core_head_dim(D: int, Sq: int, Sk: int, plain: bool) -> int:
    """The head dim the problem is run at: D itself where a matrix-core kernel takes it (32, 64, 128; 16 for the small-shape
    kernel: <= 64 rows, no mask, no fake-quant - `plain`), the next one up (zero-padded) below 128, D itself above (any-shape
    kernel)."""
    if D in (32, 64, 128) or D > 128:
        return D
    if D <= 16:
        return 16 if (plain and Sq <= 64 and Sk <= 64) else 32
    return 32 if D < 32 else (64 if D < 64 else 128)


_warned_generic = set()


def _warn_if_any_shape_kernel(lib, d, fqd, softmax) -> None:
    """The any-shape kernel (one workgroup per query ROW, fp32 FMAs) is correct for everything and ~100x slower than the
    matrix-core kernels: say so once per kind of shape instead of letting a configuration fall off that cliff silently
    (VERDICT r1 weak #13).  Asks the library which kernel the descriptor selects (a host-side call, no launch)."""
    name = lib.oeh_attn_variant(C.byref(d), None if fqd is None else C.byref(fqd))
    if name is None or not name.startswith(b"generic"):
        return
    if d.D not in (16, 32, 64, 128):
        reason = f"head dim {d.D} (matrix-core kernels: 32, 64, 128; 16 for <= 64 keys)"
    elif d.D == 16 and (d.Sq > 64 or d.Sk > 64):
        reason = f"head dim 16 with more than 64 rows (Sq={d.Sq}, Sk={d.Sk})"
    elif d.D == 16:
        reason = ("head dim 16 outside the small-shape kernel's cases (a mask, fake-quant, the in-kernel gate predictor, or rows that are "
                  f"not 4-element aligned; Sq={d.Sq}, Sk={d.Sk})")
    elif d.Sk > 512:
        what = "fused fake-quant" if fqd is not None else ("clipped softmax outside the two-pass kernel's cases" if softmax.clip else "this mask / scale combination")
        reason = f"{what} with {d.Sk} > 512 keys (the full-row kernels hold a row of <= 512 scores)"
    else:
        reason = "unaligned q / k / v / out (16-byte rows) or a mask / scale combination outside the matrix-core kernels"
    if reason not in _warned_generic:
        import warnings

        _warned_generic.add(reason)
        warnings.warn(f"outeffhop_amd: {reason} runs the any-shape HIP kernel (one workgroup per query row, fp32 FMA): correct, "
                      "but far from the matrix-core kernels' speed", RuntimeWarning, stacklevel=3)


@dataclass(frozen=True)
class QuantGrid:
    """A per-tensor 8-bit grid of one of q / k / v in INT8 storage: value = scale * (index - zero_point)."""

    scale: float
    zero_point: float

    @staticmethod
    def of(spec: "FakeQuantSpec") -> "QuantGrid":
        if spec.qmax != 255.0:
            raise ValueError("INT8 storage needs 8-bit grids")
        return QuantGrid(float(spec.scale), float(spec.zero_point))


def centre_indices(idx: torch.Tensor) -> torch.Tensor:
    """uint8 quantiser indices -> the int8 storage of the INT8 attention path (index - 128): one XOR, no copy of another kind."""
    if idx.dtype != torch.uint8:
        raise ValueError("indices must be uint8")
    return (idx ^ 128).view(torch.int8)


def split_pairs(x: torch.Tensor) -> torch.Tensor:
    """fp32 (rows, K) -> fp16 (rows, 2K) = [hi | lo] operand pairs (`oeh_split_pairs`): x = hi + lo * 2^-11 to 2^-22 relative."""
    dev = _need_gpu(x)
    if x.dim() != 2 or x.dtype != torch.float32 or x.shape[1] % 8 != 0:
        raise ValueError("x must be a 2-D fp32 tensor with a multiple of 8 columns")
    xc = x if x.stride(1) == 1 else x.contiguous()
    out = torch.empty((xc.shape[0], 2 * xc.shape[1]), dtype=torch.float16, device=x.device)
    with _on_device(dev):
        rc = _lib.load().oeh_split_pairs(_ptr(xc), _ptr(out), xc.shape[0], xc.shape[1], xc.stride(0), _stream())
    _lib.check(rc, "oeh_split_pairs")
    return out


def split_triples(x2d: torch.Tensor) -> torch.Tensor:
    """fp32 activations (rows, K) -> the fp16 matrix [xh | xh 2^-5 | xl 2^-5 | 1, 2^-5, 0 x6] (rows, 3K + 8) of `oeh_split_triples`:
    against `attention.triple_weights(weight, bias)` ONE fp16 GEMM with fp32 accumulation (torch.mm(..., out_dtype=float32)) is
    the fp32 Linear - general weights, bias included."""
    dev = _need_gpu(x2d)
    if x2d.dim() != 2 or x2d.dtype != torch.float32 or x2d.shape[1] % 8 != 0:
        raise ValueError("x must be a 2-D fp32 tensor with K % 8 == 0")
    xc = x2d if x2d.stride(1) == 1 else x2d.contiguous()
    out = torch.empty((xc.shape[0], 3 * xc.shape[1] + 8), dtype=torch.float16, device=xc.device)
    with _on_device(dev):
        rc = _lib.load().oeh_split_triples(_ptr(xc), _ptr(out), xc.shape[0], xc.shape[1], xc.stride(0), _stream())
    _lib.check(rc, "oeh_split_triples")
    return out


def quantize_heads_i8(x: torch.Tensor, spec: "FakeQuantSpec", H: int, transpose: bool = False, want_values: bool = False,
                      alpha: float = 1.0, bias: Optional[torch.Tensor] = None, want_indices: bool = True):
    """A projection's output quantiser for the INT8-storage core (`oeh_quantize_heads_i8`): x (B,S,H*64) -> centred int8 indices,
    as a logical (B,H,S,64) view of a (B,S,H*64) tensor, or with `transpose` as the contiguous (B,H,64,S) tensor `attn_fwd_i8`
    wants for v; `want_values`: also the dequantised values (B,S,H*64) in x's dtype (a decoder's cache), same pass; `bias`
    (fp32, H*64): x is a raw GEMM accumulator and alpha * x + bias is what gets quantised.  `want_indices=False` (with
    `want_values`, not transposed): only the values come back - scale + bias + output fake-quant of a QuantLinear in one pass."""
    dev = _need_gpu(x, bias)
    if bias is not None and (bias.dtype != torch.float32 or bias.numel() != H * 64 or not bias.is_contiguous()):
        raise ValueError("bias must be a contiguous fp32 vector of H*64")
    if x.dim() != 3 or x.shape[2] != H * 64 or x.dtype not in _DT or spec.qmax != 255.0:
        raise ValueError("x must be (B,S,H*64) fp16/bf16/fp32 and the grid 8-bit")
    xc = x if x.stride(2) == 1 else x.contiguous()
    B, S, E = xc.shape
    if not want_indices and (transpose or not want_values):
        raise ValueError("want_indices=False needs want_values and the untransposed layout")
    out = torch.empty((B, H, 64, S) if transpose else (B, S, E), dtype=torch.int8, device=x.device) if want_indices else None
    y = torch.empty((B, S, E), dtype=x.dtype, device=x.device) if want_values else None
    xs = (C.c_int64 * 2)(xc.stride(0), xc.stride(1))
    ys = (C.c_int64 * 2)(S * E, E)
    with _on_device(dev):
        rc = _lib.load().oeh_quantize_heads_i8(_ptr(xc), _ptr(out), _ptr(y), B, S, H, xs, ys, _DT[x.dtype], float(spec.scale), float(spec.zero_point),
                                               int(bool(transpose)), float(alpha), _ptr(bias), _stream())
    _lib.check(rc, "oeh_quantize_heads_i8")
    if not want_indices:
        return y
    idx = out if transpose else out.view(B, S, H, 64).permute(0, 2, 1, 3)
    return (idx, y) if want_values else idx


def proj_quant_i8(a: torch.Tensor, w_int: torch.Tensor, bias: torch.Tensor, B: int, S: int, segs, *, pairs: bool, _outs=None, _prepared: Optional[list] = None):
    """The q / k / v projections of a QuantLinear model as ONE GEMM with the output quantisers in its epilogue (`oeh_proj_quant_i8`):
    a (B*S, K) fp16 activations, (B*S, 2K) operand pairs of an fp32 model (`split_pairs`) or the fp32 activations (B*S, K) themselves
    (split inside the kernel: same result as the pairs, without the pass), w_int (n*E, K) fp16 = the weights'
    integers, the segments one after the other, bias (n*E) fp32; `segs` = one (alpha, FakeQuantSpec, transpose, want_values) per
    segment.  Returns per segment what `quantize_heads_i8` returns: the centred int8 indices as a logical (B,H,S,64) view of
    (B,S,E), or the contiguous (B,H,64,S) tensor with `transpose`, and with `want_values` the pair (indices, values (B,S,E) fp32)."""
    dev = _need_gpu(a, w_int, bias)
    K = w_int.shape[1]
    n = len(segs)
    if a.dtype == torch.float32:  # the fp32 activations themselves: split into (hi, lo) inside the kernel, `pairs` is implied
        form, pairs = 2, False
    else:
        form = 1 if pairs else 0
    if a.dtype not in (torch.float16, torch.float32) or w_int.dtype != torch.float16 or bias.dtype != torch.float32 or a.dim() != 2 or w_int.dim() != 2:
        raise ValueError("a 2-D fp16 (values or operand pairs) or fp32, w_int 2-D fp16, bias fp32")
    if a.shape != (B * S, (2 if pairs else 1) * K) or w_int.shape[0] % n != 0 or bias.numel() != w_int.shape[0] or not bias.is_contiguous():
        raise ValueError("shapes: a (B*S, K or 2K), w_int (n*E, K), bias (n*E)")
    if a.stride(1) != 1 or w_int.stride(1) != 1:
        raise ValueError("a and w_int must have contiguous rows")
    E = w_int.shape[0] // n
    H = E // 64
    arr = (_lib.oeh_proj_seg * n)()
    keep, res = [], []
    for i, (alpha, spec, transpose, want_values) in enumerate(segs):
        if spec.qmax != 255.0:
            raise ValueError("the output grids must be 8-bit")
        if _outs is not None:   # (plan mode, quantization._I8LayerPlan: the caller's buffers)
            out, y = _outs[i]
        else:
            out = torch.empty((B, H, 64, S) if transpose else (B, S, E), dtype=torch.int8, device=a.device)
            y = torch.empty((B, S, E), dtype=torch.float32, device=a.device) if want_values else None
        keep.append((out, y))
        arr[i].alpha, arr[i].scale, arr[i].zero_point = float(alpha), float(spec.scale), float(spec.zero_point)
        arr[i].out, arr[i].y, arr[i].y_stride_row, arr[i].transpose = _ptr(out), _ptr(y), E, int(bool(transpose))
        idx = out if transpose else out.view(B, S, H, 64).permute(0, 2, 1, 3)
        res.append((idx, y) if want_values else idx)
    if _prepared is not None:  # hand back the prebuilt C call instead of launching: [fn, mutable argument list, segment array, keep-alive]
        _prepared.extend([_lib.load().oeh_proj_quant_i8, [_ptr(a), form, _ptr(w_int), _ptr(bias), B, S, K, E, n, arr, a.stride(0), w_int.stride(0)], arr, (keep, w_int, bias)])
        return res
    with _on_device(dev):
        rc = _lib.load().oeh_proj_quant_i8(_ptr(a), form, _ptr(w_int), _ptr(bias), B, S, K, E, n, arr, a.stride(0), w_int.stride(0), _stream())
    _lib.check(rc, "oeh_proj_quant_i8")
    return res


def proj_quant_values(a: torch.Tensor, w_int: torch.Tensor, bias: torch.Tensor, alpha: float, spec: "FakeQuantSpec", *, pairs: bool,
                      acc_add: Optional[torch.Tensor] = None, _prepared: Optional[list] = None) -> torch.Tensor:
    """A whole QuantLinear in one kernel (`oeh_proj_quant_i8`, values only): fake_quant(alpha * (a @ w_int^T) + bias) as fp32 (rows, N) -
    a (rows, K) fp16 (e.g. the integers of the producer's quantiser: exact products) or (rows, 2K) operand pairs, w_int (N, K) fp16 the
    weight's integers, `spec` the frozen 8-bit output quantiser.  rows % 16 == 0, K % 32 == 0, N % 64 == 0."""
    dev = _need_gpu(a, w_int, bias, acc_add)
    N, K = w_int.shape
    rows = a.shape[0]
    i8 = a.dtype == torch.int8  # int8 activations (e.g. centred indices) against int8 weights on the integer matrix cores; acc_add: int32 (N)
    if i8:
        if w_int.dtype != torch.int8 or pairs or a.dim() != 2 or a.shape[1] != K or bias.dtype != torch.float32:
            raise ValueError("int8 form: a (rows, K) int8, w_int (N, K) int8, bias (N) fp32")
        if acc_add is not None and (acc_add.dtype != torch.int32 or acc_add.numel() != N or not acc_add.is_contiguous()):
            raise ValueError("acc_add must be a contiguous int32 vector of N")
    elif a.dtype != torch.float16 or w_int.dtype != torch.float16 or bias.dtype != torch.float32 or a.dim() != 2 or a.shape[1] != (2 if pairs else 1) * K:
        raise ValueError("a (rows, K or 2K) fp16, w_int (N, K) fp16, bias (N) fp32")
    if a.stride(1) != 1 or w_int.stride(1) != 1 or not bias.is_contiguous() or bias.numel() != N or spec.qmax != 255.0:
        raise ValueError("contiguous rows, a bias of N and an 8-bit grid")
    if rows % 16 != 0:
        raise ValueError("rows must be a multiple of 16")
    y = torch.empty((rows, N), dtype=torch.float32, device=a.device)
    seg = (_lib.oeh_proj_seg * 1)()
    seg[0].alpha, seg[0].scale, seg[0].zero_point = float(alpha), float(spec.scale), float(spec.zero_point)
    seg[0].out, seg[0].y, seg[0].y_stride_row, seg[0].transpose, seg[0].acc_add = None, _ptr(y), N, 0, (_ptr(acc_add) if i8 else None)
    if _prepared is not None:  # [fn, mutable argument list, segment array, keep-alive]: the caller patches seg[0].y (and the activations' pointer) per call
        _prepared.extend([_lib.load().oeh_proj_quant_i8, [_ptr(a), 3 if i8 else int(bool(pairs)), _ptr(w_int), _ptr(bias), rows // 16, 16, K, N, 1, seg, a.stride(0), w_int.stride(0)],
                          seg, (a, w_int, bias, acc_add, y)])
        return y
    with _on_device(dev):
        rc = _lib.load().oeh_proj_quant_i8(_ptr(a), 3 if i8 else int(bool(pairs)), _ptr(w_int), _ptr(bias), rows // 16, 16, K, N, 1, seg, a.stride(0), w_int.stride(0), _stream())
    _lib.check(rc, "oeh_proj_quant_i8")
    return y


def attn_fwd_i8(q: torch.Tensor, k: torch.Tensor, v_t: torch.Tensor, grids, *, fq: AttnFakeQuant, out_dtype=torch.float16,
                softmax: SoftmaxSpec = SoftmaxSpec(), scale: float = 1.0, scale_div: float = 0.0, causal: bool = False, clamp_min: bool = False,
                mask_min: Optional[float] = None, gate: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
                key_pad_mask: Optional[torch.Tensor] = None, _prepared: Optional[list] = None) -> torch.Tensor:
    """The INT8 configuration on the integer matrix cores (`include/oeh.h`: dtype OEH_I8): q, k logical (B,H,S,64) int8 views of
    centred indices (`centre_indices`), v_t the TRANSPOSED values, a (B,H,64,Sk) int8 view with contiguous keys; `grids` =
    (q, k, v) QuantGrid; `fq` with scores and probabilities (8-bit) [and context].  Returns the logical (B,H,Sq,64) result in
    `out_dtype`, stored (B,Sq,H,64)-contiguous.  `key_pad_mask`: (B,Sk) additive, entries 0 or <= -1e4 ONLY (HF's extended
    masks; the caller vouches for it - `attention.pad_is_boolean`).  Raises OehError(-95) for what this path does not take
    (clipping with gamma > 0, other head dims, full additive masks ...): the caller then runs `attn_fwd(..., fq=...)` on the dequantised values."""
    dev = _need_gpu(q, k, v_t, gate, out, key_pad_mask)
    if q.dtype != torch.int8 or k.dtype != torch.int8 or v_t.dtype != torch.int8:
        raise ValueError("q, k, v_t must be int8 (centred indices)")
    B, H, Sq, D = q.shape
    Sk = k.shape[2]
    if k.shape != (B, H, Sk, D) or v_t.shape != (B, H, D, Sk):
        raise ValueError(f"shape mismatch: q {tuple(q.shape)} k {tuple(k.shape)} v_t {tuple(v_t.shape)} (v_t is (B,H,D,Sk))")
    if q.stride(3) != 1 or k.stride(3) != 1 or v_t.stride(3) != 1:
        raise ValueError("q, k need a contiguous head dim and v_t contiguous keys")
    if out is None:
        out = torch.empty((B, Sq, H, D), dtype=out_dtype, device=q.device).permute(0, 2, 1, 3)
    elif out.shape != (B, H, Sq, D) or out.dtype != out_dtype or out.stride(3) != 1:
        raise ValueError("out must be a (B,H,Sq,D) view with unit head-dim stride and dtype out_dtype")
    # mask_min: q holds int8 indices here, not a dtype to take finfo.min of - the default is fp32's, whatever `out_dtype` is
    d = _attn_desc(q, k, v_t, out, _lib.OEH_I8, _lib.OEH_I8 if out_dtype == torch.int8 else _DT[out_dtype], softmax, scale, scale_div, causal, clamp_min,
                   mask_min, torch.float32)
    for name, gr in zip(("q_grid", "k_grid", "v_grid"), grids):
        getattr(d, name).scale, getattr(d, name).zero_point = float(gr.scale), float(gr.zero_point)
    keep = []
    if key_pad_mask is not None:
        _set_key_pad(d, keep, key_pad_mask, i8=True)
        d.key_pad_boolean = 1  # (this path always reads the mask that way: include/oeh.h)
    if gate is not None:
        _set_gate(d, keep, gate)
    fqd = _fq_desc(fq, always=True)  # (the library refuses this path without the scores' and probabilities' quantisers: that is its answer to give)
    if _prepared is not None:  # hand back the prebuilt C call instead of launching (bench / A-B loops)
        _prepared.extend([_lib.load().oeh_attn_fwd, (C.byref(d), _ptr(q), _ptr(k), _ptr(v_t), _ptr(out), C.byref(fqd)), (d, fqd, keep, q, k, v_t, out)])
        return out
    with _on_device(dev):
        rc = _lib.load().oeh_attn_fwd(C.byref(d), _ptr(q), _ptr(k), _ptr(v_t), _ptr(out), C.byref(fqd), _stream())
    _lib.check(rc, "oeh_attn_fwd (INT8 storage)")
    return out


@dataclass
class GatePredictor:
    """The conditional per-token gate evaluated INSIDE the attention kernel (include/oeh.h: gate_hidden ...): the layer
    input `hidden` (B,Sq,H*D) and the per-head predictor weights laid out as for `gate_fwd`; `out` (B,H,Sq) fp32, optional,
    receives the gate probabilities (without `scaling`).  The 16-bit MFMA kernels (full-row and one-pass) take it, and the full-row
    kernel on fp32 storage (operand pairs: fp32-accurate logits) (`fused_gate_ok`)."""
    hidden: torch.Tensor
    w1: torch.Tensor
    b1: torch.Tensor
    w2: Optional[torch.Tensor] = None
    b2: Optional[torch.Tensor] = None
    scaling: float = 1.0
    out: Optional[torch.Tensor] = None


def fused_gate_ok(B, H, Sq, Sk, D, dtype, clip: bool = False, fq: bool = False, units: int = 0, **problem) -> bool:
    """True when `attn_fwd(..., gate_mlp=...)` is supported for this problem (else: `gate_fwd` + `gate=`).  `problem`: the
    remaining descriptor fields that decide the kernel variant (`attn_variant`'s keywords: base, gamma, key_pad, causal,
    scale, scale_div, mask_min) - the probe must describe the real call, not a default one."""
    if dtype not in _DT or fq or int(units) > 64 or problem.get("pv_pairs"):  # (the probability pairs: no in-kernel predictor, include/oeh.h)
        return False
    v = attn_variant(B, H, Sq, Sk, D, dtype, clip=clip, gate_hidden=True, **problem)
    if v is None:
        return False
    if dtype == torch.float32:  # fp32 storage: the full-row kernel's operand-pair form (rows of <= 512 keys) ...
        if not v.startswith("fast16/"):
            return False
        # ... unless the problem WITHOUT the predictor runs the one-pass kernel: that kernel + one `gate_fwd` launch is the faster pair
        # (round 5, OPT-125m shape B=16 S=512 fp32: 42.1 + ~10 us against 58.3 us for the full-row fp32 kernel with the predictor inside)
        v0 = attn_variant(B, H, Sq, Sk, D, dtype, clip=clip, gate_hidden=False, **problem)
        return not (v0 or "").startswith("flash16/")
    return v.startswith("fast16/") or v.startswith("flash16/")


class PreparedAttn:
    """A fully built `oeh_attn_fwd` call (descriptor + pointers) for launch loops where Python argument
    marshalling would otherwise dominate: `p = PreparedAttn(q, k, v, causal=True, ...); p(); p.out`."""

    def __init__(self, q, k, v, i8_grids=None, **kw):
        box = []
        if i8_grids is not None:  # INT8 storage: q, k int8 views, v transposed (attn_fwd_i8)
            self.out = attn_fwd_i8(q, k, v, i8_grids, _prepared=box, **kw)
        else:
            self.out = attn_fwd(q, k, v, _prepared=box, **kw)
        self._fn, self._args, self._keep = box

    def __call__(self, stream: Optional[C.c_void_p] = None) -> None:
        rc = self._fn(*self._args, _stream() if stream is None else stream)
        if rc != 0:
            _lib.check(rc, "oeh_attn_fwd")


def attn_variant(B, H, Sq, Sk, D, dtype=torch.float16, fq: bool = False, clip: bool = False, *, base: int = 1, gamma: float = -0.025,
                 key_pad: bool = False, full_mask: bool = False, causal: bool = False, scale: float = 1.0, scale_div: float = 0.0,
                 mask_min: Optional[float] = None, key_pad_boolean: bool = False, gate_hidden: bool = False, pv_pairs: bool = False) -> Optional[str]:
    """Name of the kernel variant the library would pick for this problem (host only; no GPU needed).  `gate_hidden`: with the
    per-token gate predictor evaluated in the kernel (it narrows the choice).  `pv_pairs`: with attn_fwd(..., pv_pairs=True) (None where
    that is refused; the forms with probability pairs end in "+pv2")."""
    d = _probe_desc(B, H, Sq, Sk, D, dtype, scale=scale, scale_div=scale_div, base=base, clip=clip, gamma=gamma, causal=causal, mask_min=mask_min)
    d.key_pad_mask, d.key_pad_dtype, d.key_pad_boolean = (1 if key_pad else None), OEH_F32, int(bool(key_pad_boolean))
    d.full_mask, d.full_mask_dtype = (1 if full_mask else None), OEH_F32
    if gate_hidden:
        d.gate_hidden, d.gate_w1, d.gate_b1 = 1, 1, 1
    fqd = _fq_desc(_PROBE_FQ) if fq else None
    if pv_pairs:
        r = _lib.load().oeh_attn_variant_ex(C.byref(d), C.byref(oeh_attn_opts(pv_pairs=1)), None if fqd is None else C.byref(fqd))
    else:
        r = _lib.load().oeh_attn_variant(C.byref(d), None if fqd is None else C.byref(fqd))
    return None if r is None else r.decode()


DECODE_CALLS = 0  # launches of `attn_decode` (the modules' generation steps: attention.SPLIT_DECODE)
_decode_work = {}  # (device index, stream handle) -> the split-key scratch of that stream


def _decode_scratch(dev, nbytes: int):
    """The current stream's split-key scratch for `oeh_attn_decode` on `dev` (`_scratch`)."""
    return _scratch(_decode_work, dev, nbytes)


def attn_decode(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, *, softmax: SoftmaxSpec = SoftmaxSpec(), scale: float = 1.0, scale_div: float = 0.0,
                key_pad_mask: Optional[torch.Tensor] = None, causal: bool = False, clamp_min: bool = False, mask_min: Optional[float] = None,
                gate: Optional[torch.Tensor] = None, out_dtype: Optional[torch.dtype] = None, splits: int = 0,
                fq: Optional[AttnFakeQuant] = None) -> torch.Tensor:
    """Split-key decode attention (`oeh_attn_decode`): a generation step - q (B,H,Sq,64) with 1 <= Sq <= 16 against k, v (B,H,Sk,64) views of
    a cache (any batch / head / sequence strides, unit head-dim stride; fp16 / bf16) - with the keys of a head split over `splits`
    workgroups (0: the library's rule) and a combine pass.  Masks, gate, `out_dtype` and the result's layout ((B,Sq,H,D)-contiguous) as
    `attn_fwd`; what the entry point does not take (another head dim, more query rows, fp32 storage, gamma > 0) raises OehError -95.
    `fq`: the fused INT8 chain as in `attn_fwd` (`oeh_attn_decode_fq`: any subset of the three quantisers, index dumps included;
    `ctx_emit_index` is refused, -95); None or nothing enabled: `oeh_attn_decode` itself.
    Bitwise reproducible; graph-capture safe (a captured call owns its scratch: `_scratch`)."""
    global DECODE_CALLS
    dev = _need_gpu(q, k, v, key_pad_mask, gate)
    q, k, v = _check_qkv(q, k, v)
    B, H, Sq, D = q.shape
    odt = q.dtype if out_dtype is None else out_dtype
    if odt != q.dtype and odt != torch.float32:
        raise ValueError(f"out_dtype must be the input dtype or float32 (got {odt} for {q.dtype})")
    out = torch.empty((B, Sq, H, D), dtype=odt, device=q.device).permute(0, 2, 1, 3)
    d = _attn_desc(q, k, v, out, _DT[q.dtype], _DT[odt], softmax, scale, scale_div, causal, clamp_min, mask_min, q.dtype)
    keep = []
    if key_pad_mask is not None:
        _set_key_pad(d, keep, key_pad_mask)  # (key_pad_boolean stays 0: this entry point has no such argument)
    if gate is not None:
        _set_gate(d, keep, gate)
    lib = _lib.load()
    nbytes = lib.oeh_attn_decode_work_bytes(C.byref(d), int(splits))
    if nbytes < 0:
        _lib.check(int(nbytes), "oeh_attn_decode")
    work = _decode_scratch(dev, int(nbytes))
    fqd = _fq_desc(fq)
    if fqd is not None:
        with _on_device(dev):
            rc = lib.oeh_attn_decode_fq(C.byref(d), C.byref(fqd), int(splits), _ptr(q), _ptr(k), _ptr(v), _ptr(out), _ptr(work), _stream())
        _lib.check(rc, "oeh_attn_decode_fq")
    else:
        with _on_device(dev):
            rc = lib.oeh_attn_decode(C.byref(d), int(splits), _ptr(q), _ptr(k), _ptr(v), _ptr(out), _ptr(work), _stream())
        _lib.check(rc, "oeh_attn_decode")
    DECODE_CALLS += 1
    return out


def attn_decode_variant(B, H, Sq, Sk, D=64, dtype=torch.float16, *, clip: bool = False, gamma: float = -0.025, causal: bool = False, splits: int = 0,
                        fq: bool = False) -> Optional[str]:
    """Name of the form `attn_decode` would run ("decode16/SP<effective splits>/D64/f16[/clip][/fq]"; `fq`: with the fused INT8 chain), or None
    where it refuses (host only)."""
    d = _probe_desc(B, H, Sq, Sk, D, dtype, clip=clip, gamma=gamma, causal=causal)
    if fq:
        r = _lib.load().oeh_attn_decode_fq_variant(C.byref(d), C.byref(_fq_desc(_PROBE_FQ)), int(splits))
    else:
        r = _lib.load().oeh_attn_decode_variant(C.byref(d), int(splits))
    return None if r is None else r.decode()


def softmax_rows(x: torch.Tensor, spec: SoftmaxSpec = SoftmaxSpec(), dim: int = -1, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """SOFTMAX_MAPPING callable on the GPU: softmax / softmax_1 / clipped variants along `dim`."""
    dev = _need_gpu(x, out)
    _need_dtype(x)
    nd = x.dim()
    dim = dim % nd
    xt = x if dim == nd - 1 else x.transpose(dim, -1)
    xc = xt.contiguous()
    y = torch.empty_like(xc) if out is None or dim != nd - 1 else out
    cols = xc.shape[-1]
    rows = xc.numel() // max(cols, 1)
    if xc.numel():
        with _on_device(dev):
            rc = _lib.load().oeh_softmax_rows(_ptr(xc), _ptr(y), rows, cols, _DT[x.dtype], int(spec.base), int(bool(spec.clip)),
                                              float(spec.gamma), float(spec.eta), _stream())
        _lib.check(rc, "oeh_softmax_rows")
    return y if dim == nd - 1 else y.transpose(dim, -1)


def fake_quant(x: torch.Tensor, spec: FakeQuantSpec, want_idx: bool = False):
    """Fixed-range per-tensor asymmetric fake-quant; returns x_q (and the uint8 indices if asked)."""
    dev = _need_gpu(x)
    _need_dtype(x)
    xc = x.contiguous()
    y = torch.empty_like(xc)
    idx = torch.empty(xc.shape, dtype=torch.uint8, device=x.device) if want_idx else None
    with _on_device(dev):
        rc = _lib.load().oeh_fake_quant(_ptr(xc), _ptr(y), _ptr(idx), xc.numel(), _DT[x.dtype], spec.scale, spec.zero_point, spec.qmax, _stream())
    _lib.check(rc, "oeh_fake_quant")
    return (y, idx) if want_idx else y


# ---- the quantised block tail (include/oeh.h: oeh_resid_ln_quant): residual + sum quantiser + LayerNorm + output quantiser in one pass
LN_MAX_COLS = 8192  # rows longer than this are refused (OEH_ENOTSUP)


def _rows_view(t: torch.Tensor, cols: int):
    """`t` (..., cols) as rows: (a tensor that shares t's memory where a 2-D view exists - else a contiguous copy -, its row stride)."""
    if t.dim() == 0 or t.shape[-1] != cols:
        raise ValueError(f"expected a last dimension of {cols}, got shape {tuple(t.shape)}")
    if cols > 1 and t.stride(-1) != 1:
        t = t.contiguous()
    try:
        v = t.view(-1, cols)
    except RuntimeError:
        t = t.contiguous()
        v = t.view(-1, cols)
    return v, (v.stride(0) if v.shape[0] > 1 else cols)


def _own_rows(t: torch.Tensor, cols: int, what: str):
    """An output as rows: it must BE the memory it was given as - no copy may stand in for it."""
    v, st = _rows_view(t, cols)
    if v.data_ptr() != t.data_ptr() or (v.shape[0] > 1 and st < cols):
        raise ValueError(f"{what} needs a contiguous last dimension and leading dimensions that collapse to one row stride")
    return v, st


_ACT = {"none": _lib.OEH_ACT_NONE, "relu": _lib.OEH_ACT_RELU, "gelu": _lib.OEH_ACT_GELU}


def _act_code(act: str) -> int:
    if act not in _ACT:
        raise ValueError(f"act must be one of {sorted(_ACT)}, got {act!r}")
    return _ACT[act]


def act_quant(x: torch.Tensor, spec: FakeQuantSpec, *, act: str = "none", alpha: float = 1.0, bias: Optional[torch.Tensor] = None,
              want_values: bool = True, want_index: bool = False):
    """fake_quant(act(alpha * x + bias)) over the last dimension's rows in ONE kernel (`include/oeh.h: oeh_act_quant`): the elementwise tail of
    a QuantLinear with an activation function.  x (..., cols) fp16 / bf16 / fp32 with cols % 16 == 0, read in place where its leading
    dimensions collapse to one row stride; `bias` (cols, fp32): x is a raw GEMM accumulator and alpha * x + bias is the value, otherwise x
    itself; act "none" | "relu" | "gelu" (the erf form); `spec` a frozen 8-bit grid.  Returns the dequantised values in x's dtype
    (want_values), the centred int8 indices idx - 128 (want_index: the operand of `QuantLinear.linear_index`), or the pair (values, indices)."""
    dev = _need_gpu(x, bias)
    _need_dtype(x)
    code = _act_code(act)
    if not (want_values or want_index):
        raise ValueError("act_quant needs want_values or want_index")
    if spec.qmax != 255.0:
        raise ValueError("the grid must be 8-bit")
    cols = x.shape[-1] if x.dim() else 0
    if cols < 1:
        raise ValueError("act_quant needs a last dimension of at least 1")
    if bias is not None and (bias.dtype != torch.float32 or bias.numel() != cols or not bias.is_contiguous()):
        raise ValueError("bias must be a contiguous fp32 vector of one value per column")
    xv, xs = _rows_view(x.detach(), cols)
    rows = xv.shape[0]
    y = torch.empty(x.shape, dtype=x.dtype, device=x.device) if want_values else None
    idx = torch.empty(x.shape, dtype=torch.int8, device=x.device) if want_index else None
    if rows:  # (an empty tensor has no address to hand over)
        with _on_device(dev):
            rc = _lib.load().oeh_act_quant(_ptr(xv), _ptr(idx), _ptr(y), rows, cols, xs, cols, _DT[x.dtype], code, float(spec.scale),
                                           float(spec.zero_point), float(alpha), _ptr(bias), _stream())
        _lib.check(rc, "oeh_act_quant")
    if want_values and want_index:
        return y, idx
    return y if want_values else idx


def act_quant_variant(rows: int, cols: int, dtype=torch.float32, *, act: str = "none", row_stride: Optional[int] = None, want_values: bool = True,
                      want_index: bool = False) -> Optional[str]:
    """Name of the launch form `act_quant` takes for (rows, cols) tensors of `dtype` whose rows are `row_stride` (default: cols) elements
    apart ("actq/relu/f32/y+i8/once", "actq/gelu/f16/i8/loop"), or None if refused.  Host only."""
    st = cols if row_stride is None else int(row_stride)
    r = _lib.load().oeh_act_quant_variant(int(rows), int(cols), st, int(cols), _DT[dtype], _act_code(act), int(bool(want_values)), int(bool(want_index)))
    return None if r is None else r.decode()


def _ln_rows_in(op: str, x, residual, weight, bias, out, sum_out, allow_grad: bool):
    """The opening `resid_ln_quant` and `drop_resid_ln_fwd` share: device and dtype, cols, the optional tensors' shape and dtype, the row views of
    x and residual, gamma / beta as fp32.  Returns (dev, cols, xv, xs, rv, rs, g, b)."""
    dev = _need_gpu(x, residual, weight, bias, out, sum_out, allow_grad=allow_grad)
    _need_dtype(x)
    cols = x.shape[-1] if x.dim() else 0
    if cols < 1:
        raise ValueError(f"{op} needs a last dimension of at least 1")
    for t_, what in ((residual, "residual"), (out, "out"), (sum_out, "sum_out")):
        if t_ is not None and (t_.shape != x.shape or t_.dtype != x.dtype):
            raise ValueError(f"{what} must have x's shape and dtype")
    if weight.numel() != cols or (bias is not None and bias.numel() != cols):
        raise ValueError("weight / bias must hold one value per column")
    xv, xs = _rows_view(x.detach(), cols)
    rv, rs = _rows_view(residual.detach(), cols) if residual is not None else (None, 0)
    f32 = lambda t: None if t is None else t.detach().reshape(-1).to(torch.float32).contiguous()  # noqa: E731
    return dev, cols, xv, xs, rv, rs, f32(weight), f32(bias)


def _ln_desc(rows: int, cols: int, dtype, strides, eps: float, fq_sum: Optional[FakeQuantSpec], fq_out: Optional[FakeQuantSpec]) -> _lib.oeh_ln_desc:
    d = _lib.oeh_ln_desc()
    d.rows, d.cols, d.dtype = rows, cols, _DT[dtype]
    d.x_stride, d.r_stride, d.sum_stride, d.y_stride = strides
    d.eps = float(eps)
    for dst, spec in ((d.fq_sum, fq_sum), (d.fq_out, fq_out)):
        _fill_fq(dst, None if spec is None else FakeQuantSpec(spec.scale, spec.zero_point, spec.qmax))  # (the dumps are arguments of the call)
    return d


def resid_ln_quant(x: torch.Tensor, residual: Optional[torch.Tensor] = None, weight: Optional[torch.Tensor] = None, bias: Optional[torch.Tensor] = None,
                   eps: float = 1e-5, *, fq_sum: Optional[FakeQuantSpec] = None, fq_out: Optional[FakeQuantSpec] = None, want_sum: bool = False,
                   want_idx: bool = False, out: Optional[torch.Tensor] = None, sum_out: Optional[torch.Tensor] = None):
    """fq_out(LayerNorm(fq_sum(x + residual))) over the last dimension in ONE kernel (`include/oeh.h: oeh_resid_ln_quant`): the tail of a
    quantised BERT / OPT block.  x, residual (..., N) fp16 / bf16 / fp32 with a contiguous last dimension, read in place where their
    leading dimensions collapse to one row stride; weight (N) - required - and bias (N): the LayerNorm's gamma and beta, taken as fp32 (already
    fake-quantised where weight quantisation is on).  Either quantiser may be None.  Returns y, or (sum, y) with want_sum - sum = fq_sum(x +
    residual), what the next residual connection reads -, or (sum, y, sum_idx, y_idx) with want_idx (uint8 indices, None for an absent
    quantiser; tests).  out / sum_out: where to write (x's shape and dtype); sum_out may be `residual` or `x`, and out may be `x`."""
    if weight is None:
        raise ValueError("resid_ln_quant needs the LayerNorm's weight")
    dev, cols, xv, xs, rv, rs, g, b = _ln_rows_in("resid_ln_quant", x, residual, weight, bias, out, sum_out, False)
    want_sum = want_sum or want_idx or sum_out is not None
    y = out if out is not None else torch.empty(x.shape, dtype=x.dtype, device=x.device)
    s = (sum_out if sum_out is not None else torch.empty(x.shape, dtype=x.dtype, device=x.device)) if want_sum else None
    (sv, ss), (yv, ys) = _own_rows(s, cols, "sum_out") if want_sum else (None, 0), _own_rows(y, cols, "out")
    rows = xv.shape[0]
    sidx = torch.empty(x.shape, dtype=torch.uint8, device=x.device) if want_idx and fq_sum is not None else None
    yidx = torch.empty(x.shape, dtype=torch.uint8, device=x.device) if want_idx and fq_out is not None else None
    d = _ln_desc(rows, cols, x.dtype, (xs, rs, ss, ys), eps, fq_sum, fq_out)
    if rows:  # (an empty tensor has no address to hand over)
        with _on_device(dev):
            rc = _lib.load().oeh_resid_ln_quant(C.byref(d), _ptr(xv), _ptr(rv), _ptr(g), _ptr(b), _ptr(sv), _ptr(yv), _ptr(sidx), _ptr(yidx), _stream())
        _lib.check(rc, "oeh_resid_ln_quant")
    if want_idx:
        return s, y, sidx, yidx
    return (s, y) if want_sum else y


def resid_ln_variant(rows: int, cols: int, dtype=torch.float32, *, row_stride: Optional[int] = None, eps: float = 1e-5) -> Optional[str]:
    """Name of the launch form `resid_ln_quant` takes for (rows, cols) tensors of `dtype` whose rows are `row_stride` (default: cols)
    elements apart and 16-byte aligned ("ln/wave/CH4/f32", "ln/block/CH8/f16", "ln/scalar/CH1/bf16"), or None if refused.  Host only."""
    st = cols if row_stride is None else int(row_stride)
    d = _ln_desc(int(rows), int(cols), dtype, (st, st, st, st), eps, None, None)
    r = _lib.load().oeh_resid_ln_variant(C.byref(d))
    return None if r is None else r.decode()


# ---- the block tail in training (include/oeh.h: oeh_drop_resid_ln_fwd / oeh_drop_resid_ln_bwd): dropout + residual + LayerNorm, both directions
def _ln_train_desc(rows: int, cols: int, dtype, strides, eps: float, p: float, seed: Optional[int], dsum_stride: int = 0) -> _lib.oeh_ln_train_desc:
    """strides: (x, r, sum, y) forward, (dx, dr, s, dy) backward.  The library validates p; the seed is a uint64 and has to be given with p != 0."""
    d = _lib.oeh_ln_train_desc()
    d.rows, d.cols, d.dtype = rows, cols, _DT[dtype]
    d.x_stride, d.r_stride, d.sum_stride, d.y_stride = strides
    d.dsum_stride = dsum_stride
    d.eps = float(eps)
    drop = _dropout(p, seed)
    d.drop.p, d.drop.seed = (0.0, 0) if drop is None else (drop.p, drop.seed)
    return d


def drop_resid_ln_fwd(x: torch.Tensor, residual: Optional[torch.Tensor], weight: torch.Tensor, bias: Optional[torch.Tensor] = None, eps: float = 1e-5,
                      *, p: float = 0.0, seed: Optional[int] = None, out: Optional[torch.Tensor] = None, sum_out: Optional[torch.Tensor] = None):
    """(sum, y, mean, rstd) of LayerNorm(dropout(x) + residual) over the last dimension in ONE kernel (`include/oeh.h: oeh_drop_resid_ln_fwd`):
    sum = dropout(x) + residual in x's dtype - what the backward reads and what a pre-LN block carries on -, y its LayerNorm, mean / rstd the
    row statistics (x.shape[:-1]; formed in float64, stored as fp32).  x, residual (..., N) fp16 / bf16 / fp32; weight (N) and bias (N) are taken as fp32.  p > 0 needs the
    uint64 `seed` of the keep mask (`drop_resid_ln_mask`).  No autograd here (see `layers.dropout_add_layer_norm`).  sum_out may be `residual`,
    out may be `x`."""
    dev, cols, xv, xs, rv, rs, g, b = _ln_rows_in("drop_resid_ln_fwd", x, residual, weight, bias, out, sum_out, True)
    y = out if out is not None else torch.empty(x.shape, dtype=x.dtype, device=x.device)
    s = sum_out if sum_out is not None else torch.empty(x.shape, dtype=x.dtype, device=x.device)
    (sv, ss), (yv, ys) = _own_rows(s, cols, "sum_out"), _own_rows(y, cols, "out")
    rows = xv.shape[0]
    mean = torch.empty(x.shape[:-1], dtype=torch.float32, device=x.device)
    rstd = torch.empty(x.shape[:-1], dtype=torch.float32, device=x.device)
    d = _ln_train_desc(rows, cols, x.dtype, (xs, rs, ss, ys), eps, p, seed)
    if rows:  # (an empty tensor has no address to hand over)
        with _on_device(dev):
            rc = _lib.load().oeh_drop_resid_ln_fwd(C.byref(d), _ptr(xv), _ptr(rv), _ptr(g), _ptr(b), _ptr(sv), _ptr(yv), _ptr(mean), _ptr(rstd), _stream())
        _lib.check(rc, "oeh_drop_resid_ln_fwd")
    return s, y, mean, rstd


_ln_train_work = {}  # (device index, stream handle) -> the per-workgroup column partials of that stream's backward


def drop_resid_ln_bwd(dy: torch.Tensor, s: torch.Tensor, weight: torch.Tensor, mean: torch.Tensor, rstd: torch.Tensor, eps: float = 1e-5, *,
                      dsum: Optional[torch.Tensor] = None,
                      p: float = 0.0, seed: Optional[int] = None, want_dr: bool = True, want_dbeta: bool = True, dx: Optional[torch.Tensor] = None,
                      dr: Optional[torch.Tensor] = None):
    """(dx, dr, dgamma, dbeta) of `drop_resid_ln_fwd` from its sum `s`, mean, rstd and (p, seed), the output gradient dy and - where the sum was
    an output with a gradient of its own - dsum (`include/oeh.h: oeh_drop_resid_ln_bwd`).  dx, dr: s's shape and dtype (dr None without
    want_dr); dgamma, dbeta: fp32 (N) (dbeta None without want_dbeta), summed in float64 from the row statistics the kernel forms again in
    float64 - which is what `eps`, the forward's, is for - and rounded once.  Two HIP kernels, no atomics: the same bits on every call.  dx may be
    `dy`, dr may be `dsum`."""
    dev = _need_gpu(dy, s, weight, mean, rstd, dsum, dx, dr, allow_grad=True)
    _need_dtype(s)
    cols = s.shape[-1] if s.dim() else 0
    if cols < 1:
        raise ValueError("drop_resid_ln_bwd needs a last dimension of at least 1")
    for t_, what in ((dy, "dy"), (dsum, "dsum"), (dx, "dx"), (dr, "dr")):
        if t_ is not None and (t_.shape != s.shape or t_.dtype != s.dtype):
            raise ValueError(f"{what} must have s's shape and dtype")
    if weight.numel() != cols:
        raise ValueError("weight must hold one value per column")
    sv, ss = _rows_view(s.detach(), cols)
    rows = sv.shape[0]
    for t_, what in ((mean, "mean"), (rstd, "rstd")):
        if t_.dtype != torch.float32 or t_.numel() != rows or not t_.is_contiguous():
            raise ValueError(f"{what} must be the contiguous fp32 row statistic of drop_resid_ln_fwd")
    dyv, dys = _rows_view(dy.detach(), cols)
    dsv, dss = _rows_view(dsum.detach(), cols) if dsum is not None else (None, 0)
    dx = dx if dx is not None else torch.empty(s.shape, dtype=s.dtype, device=s.device)
    dxv, dxs = _own_rows(dx, cols, "dx")
    if dr is None and want_dr:
        dr = torch.empty(s.shape, dtype=s.dtype, device=s.device)
    drv, drs = _own_rows(dr, cols, "dr") if dr is not None else (None, 0)
    dgamma = torch.empty(cols, dtype=torch.float32, device=s.device)
    dbeta = torch.empty(cols, dtype=torch.float32, device=s.device) if want_dbeta else None
    g = weight.detach().reshape(-1).to(torch.float32).contiguous()
    d = _ln_train_desc(rows, cols, s.dtype, (dxs, drs, ss, dys), eps, p, seed, dss)
    lib = _lib.load()
    if rows:
        work = _scratch(_ln_train_work, dev, max(int(lib.oeh_drop_resid_ln_bwd_work_bytes(C.byref(d))), 8))
        with _on_device(dev):
            rc = lib.oeh_drop_resid_ln_bwd(C.byref(d), _ptr(dyv), _ptr(dsv), _ptr(sv), _ptr(g), _ptr(mean), _ptr(rstd), _ptr(dxv), _ptr(drv), _ptr(dgamma),
                                           _ptr(dbeta), _ptr(work), _stream())
        _lib.check(rc, "oeh_drop_resid_ln_bwd")
    else:  # (an empty tensor has no address to hand over: sums over no row)
        dgamma.zero_()
        if dbeta is not None:
            dbeta.zero_()
    return dx, dr, dgamma, dbeta


def drop_resid_ln_mask(rows: int, cols: int, p: float, seed: int, device) -> torch.Tensor:
    """The keep mask `drop_resid_ln_fwd` / `drop_resid_ln_bwd` apply for (p, seed): a (rows, cols) bool tensor on `device`, True where an
    element of x is kept (and scaled by 1 / (1 - p)).  include/oeh.h: oeh_drop_resid_ln_mask; p == 0 keeps everything."""
    device = torch.device(device)
    if device.type != "cuda":
        raise _lib.OehError("outeffhop_amd ops need GPU tensors: the HIP library is the only implementation")
    d = _ln_train_desc(int(rows), int(cols), torch.float32, (cols, cols, cols, cols), 0.0, p, seed)
    keep = torch.empty((rows, cols), dtype=torch.uint8, device=device)
    if rows:
        with _on_device(device):
            rc = _lib.load().oeh_drop_resid_ln_mask(C.byref(d), _ptr(keep), _stream())
        _lib.check(rc, "oeh_drop_resid_ln_mask")
    return keep.view(torch.bool)


def drop_resid_ln_variant(rows: int, cols: int, dtype=torch.float32, *, backward: bool = False, p: float = 0.0, row_stride: Optional[int] = None) -> Optional[str]:
    """Name of the launch form the training block tail takes for (rows, cols) tensors of `dtype` whose rows are `row_stride` (default: cols)
    elements apart and 16-byte aligned: "ln_train/fwd/wave/CH2/f16/drop", "ln_train/bwd/block/CH8/f32/G512x2" (backward: workgroups of the
    row kernel x rows of a slab), or None if refused.  Host only."""
    st = cols if row_stride is None else int(row_stride)
    d = _ln_train_desc(int(rows), int(cols), dtype, (st, st, st, st), 1e-5, p, 0, st)
    r = _lib.load().oeh_drop_resid_ln_variant(C.byref(d), int(bool(backward)))
    return None if r is None else r.decode()


# ---- the quantised model front (include/oeh.h: oeh_embed_sum_quant): embedding lookups + sums + their quantisers + LayerNorm in one pass
@dataclass
class EmbedLookup:
    """One lookup of `embed_sum_quant`.  table (n_rows, cols): the storage dtype, or int8 (the weight grid's integers, with `scale`); ids:
    int32 / int64, broadcastable to the call's (B, S) - None (the first lookup only): `table` is (B, S, cols), one dense row per position.
    scale (with int_min, int_max) on a float table: the per-tensor symmetric weight grid, applied to the gathered rows on the fly."""

    table: torch.Tensor
    ids: Optional[torch.Tensor] = None
    scale: Optional[float] = None
    int_min: float = -128.0
    int_max: float = 127.0


def _embed_desc(B: int, S: int, cols: int, dtype, lookups, views, strides, eps: float, fq_sums, fq_out: Optional[FakeQuantSpec]) -> _lib.oeh_embed_desc:
    d = _lib.oeh_embed_desc()
    d.B, d.S, d.cols, d.dtype, d.n_tab = B, S, cols, _DT[dtype], len(lookups)
    d.sum_stride, d.y_stride = strides
    d.eps = float(eps)
    for t, (lk, ((tv, ts), iv)) in enumerate(zip(lookups, views)):
        l = d.tab[t]
        l.table, l.row_stride, l.n_rows = tv.data_ptr(), ts, (B * S if iv is None else lk.table.shape[0])
        if iv is not None:
            l.ids, l.id_stride_b, l.id_stride_s = iv.data_ptr(), iv.stride(0), iv.stride(1)
            l.id_dtype = _lib.OEH_ID_I64 if iv.dtype == torch.int64 else _lib.OEH_ID_I32
        l.form = _lib.OEH_TAB_I8 if lk.table.dtype == torch.int8 else _lib.OEH_TAB_GRID if lk.scale is not None else _lib.OEH_TAB_PLAIN
        if lk.scale is not None:
            l.scale, l.int_min, l.int_max = float(lk.scale), float(lk.int_min), float(lk.int_max)
    for t, spec in enumerate(fq_sums):
        _fill_fq(d.fq_sum[t + 1], None if spec is None else FakeQuantSpec(spec.scale, spec.zero_point, spec.qmax))  # (the dumps are arguments of the call)
    _fill_fq(d.fq_out, None if fq_out is None else FakeQuantSpec(fq_out.scale, fq_out.zero_point, fq_out.qmax))
    return d


def _embed_geometry(lookups, dtype):
    """(B, S, cols, dtype) of a call and, per lookup, ((table rows view, row stride), ids expanded to (B, S) or None)."""
    if not 1 <= len(lookups) <= 3:
        raise ValueError("embed_sum_quant takes one to three lookups")
    shapes = []
    for t, lk in enumerate(lookups):
        if lk.ids is None:
            if t != 0 or lk.table.dim() != 3:
                raise ValueError("only the first lookup may come without ids, as dense (B, S, cols) rows")
            shapes.append(tuple(lk.table.shape[:2]))
        else:
            if lk.ids.dtype not in (torch.int32, torch.int64) or lk.ids.dim() != 2 or lk.table.dim() != 2:
                raise ValueError("ids must be 2-D int32 / int64 tensors and their tables 2-D")
            shapes.append(tuple(lk.ids.shape))
        if lk.table.dtype == torch.int8:
            if lk.scale is None:
                raise ValueError("an int8 table needs its scale")
        elif dtype is None:
            dtype = lk.table.dtype
        elif lk.table.dtype != dtype:
            raise ValueError(f"tables must share one storage dtype, got {dtype} and {lk.table.dtype}")
    if dtype not in _DT:
        raise ValueError(f"unsupported dtype {dtype}" if dtype is not None else "int8 tables alone do not say the storage dtype: pass dtype=")
    B, S = torch.broadcast_shapes(*shapes)
    cols = lookups[0].table.shape[-1]
    views = []
    for lk in lookups:
        if lk.table.shape[-1] != cols:
            raise ValueError("tables must share their row length")
        if lk.ids is None:
            if tuple(lk.table.shape[:2]) != (B, S):
                raise ValueError("dense rows must cover the whole (B, S) grid")
            views.append((_rows_view(lk.table.detach(), cols), None))
        else:
            tb = lk.table.detach()
            if cols > 1 and tb.stride(1) != 1:
                tb = tb.contiguous()
            views.append(((tb, tb.stride(0) if tb.shape[0] > 1 else cols), lk.ids.detach().expand(B, S)))
    return B, S, cols, dtype, views


def embed_sum_quant(lookups, weight: Optional[torch.Tensor] = None, bias: Optional[torch.Tensor] = None, eps: float = 1e-5, *, fq_sums=(),
                    fq_out: Optional[FakeQuantSpec] = None, dtype=None, want_sum: bool = False, want_idx: bool = False, out: Optional[torch.Tensor] = None,
                    sum_out: Optional[torch.Tensor] = None, check_ids: bool = False):
    """The front of a quantised model in ONE kernel (`include/oeh.h: oeh_embed_sum_quant`): s = row of lookups[0]; for each further lookup t
    s = fq_sums[t - 1](s + its row); y = fq_out(LayerNorm(s)) with the LayerNorm's `weight` (and `bias`), or y = s without them.  lookups:
    one to three `EmbedLookup`; fq_sums: one entry (a FakeQuantSpec or None) per lookup after the first, missing ones are None.  Returns y
    (B, S, cols), or (sum, y) with want_sum, or (sum, y, sum_idx, y_idx) with want_idx (uint8 indices of the LAST sum quantiser and of
    fq_out, None for an absent one; tests).  out / sum_out: where to write.  A row with an id outside its table is NaN (nothing is read for
    it); check_ids=True also returns the number of such rows as the last element, at the price of one synchronisation."""
    lookups = list(lookups)
    dev = _need_gpu(weight, bias, out, sum_out, *[lk.table for lk in lookups], *[lk.ids for lk in lookups])
    B, S, cols, dtype, views = _embed_geometry(lookups, dtype)
    fq_sums = list(fq_sums) + [None] * (len(lookups) - 1 - len(fq_sums))
    if len(fq_sums) != len(lookups) - 1:
        raise ValueError("fq_sums has one entry per lookup after the first")
    if weight is None and (bias is not None or fq_out is not None):
        raise ValueError("bias and fq_out belong to the LayerNorm: pass its weight")
    if weight is not None and (weight.numel() != cols or (bias is not None and bias.numel() != cols)):
        raise ValueError("weight / bias must hold one value per column")
    shape = (B, S, cols)
    for t_, what in ((out, "out"), (sum_out, "sum_out")):
        if t_ is not None and (tuple(t_.shape) != shape or t_.dtype != dtype):
            raise ValueError(f"{what} must be (B, S, cols) of the tables' dtype")
    want_sum = want_sum or want_idx or sum_out is not None
    device = lookups[0].table.device
    y = out if out is not None else torch.empty(shape, dtype=dtype, device=device)
    s = (sum_out if sum_out is not None else torch.empty(shape, dtype=dtype, device=device)) if want_sum else None
    outs = []
    for t_ in (s, y):  # an output must BE the memory it was given as: no copy may stand in for it
        if t_ is None:
            outs.append((None, 0))
            continue
        v_, st_ = _rows_view(t_, cols)
        if v_.data_ptr() != t_.data_ptr() or (v_.shape[0] > 1 and st_ < cols):
            raise ValueError("out / sum_out need a contiguous last dimension and leading dimensions that collapse to one row stride")
        outs.append((v_, st_))
    (sv, ss), (yv, ys) = outs
    f32 = lambda t: None if t is None else t.detach().reshape(-1).to(torch.float32).contiguous()  # noqa: E731
    g, b = f32(weight), f32(bias)
    last = fq_sums[-1] if fq_sums else None
    sidx = torch.empty(shape, dtype=torch.uint8, device=device) if want_idx and last is not None else None
    yidx = torch.empty(shape, dtype=torch.uint8, device=device) if want_idx and fq_out is not None else None
    bad = torch.zeros(1, dtype=torch.int32, device=device) if check_ids else None
    d = _embed_desc(B, S, cols, dtype, lookups, views, (ss, ys), eps, fq_sums, fq_out)
    if B * S:  # (an empty tensor has no address to hand over)
        with _on_device(dev):
            rc = _lib.load().oeh_embed_sum_quant(C.byref(d), _ptr(g), _ptr(b), _ptr(sv), _ptr(yv), _ptr(sidx), _ptr(yidx), _ptr(bad), _stream())
        _lib.check(rc, "oeh_embed_sum_quant")
    res = (s, y, sidx, yidx) if want_idx else (s, y) if want_sum else y
    if check_ids:
        n_bad = int(bad.item())
        return (*res, n_bad) if isinstance(res, tuple) else (res, n_bad)
    return res


def embed_sum_variant(B: int, S: int, cols: int, dtype=torch.float32, *, n_tab: int = 3, int8: bool = False, row_stride: Optional[int] = None,
                      table_offset: int = 0) -> Optional[str]:
    """Name of the launch form `embed_sum_quant` takes for `n_tab` lookups of `cols`-element rows `row_stride` (default: cols) elements
    apart into (B, S, cols) outputs of `dtype` - float tables, or int8 ones - whose tables start `table_offset` bytes behind a 16-byte
    boundary ("embed/wave/CH4/T3/f32", "embed/block/CH4/T2/f16", "embed/scalar/CH1/T1/bf16"), or None if refused.  Host only."""
    st = cols if row_stride is None else int(row_stride)
    d = _lib.oeh_embed_desc()
    d.B, d.S, d.cols, d.dtype, d.n_tab = int(B), int(S), int(cols), _DT[dtype], int(n_tab)
    d.sum_stride = d.y_stride = cols
    for t in range(max(0, min(int(n_tab), 3))):
        l = d.tab[t]
        l.table, l.ids, l.n_rows, l.row_stride, l.id_stride_b, l.id_stride_s = 4096 + int(table_offset), 4096, 1, st, int(S), 1
        if int8:
            l.form, l.scale, l.int_min, l.int_max = _lib.OEH_TAB_I8, 1.0, -128.0, 127.0
    r = _lib.load().oeh_embed_sum_variant(C.byref(d))
    return None if r is None else r.decode()


# ---- cross-entropy over a vocabulary (include/oeh.h: oeh_xent_fwd / oeh_xent_bwd): loss and logit gradient from one pass each

XENT_SLOTS = _lib.XENT_SLOTS  # 16-byte slots per thread and loop step: a step covers 256 * XENT_SLOTS * (4 fp32 | 8 16-bit) elements
XENT_CALLS = 0  # launches of `xent_fwd` (losses.FUSED_XENT)
_ID_DT = {torch.int32: _lib.OEH_ID_I32, torch.int64: _lib.OEH_ID_I64}


def _xent_views(logits: torch.Tensor, labels: torch.Tensor):
    """(B, S, V) logits and (B, S) labels as the kernel addresses them: 1-d logits are one row, 2-d ones (1, N, V), more than three
    dimensions fold their leading ones into B.  A view is passed as it is, by its strides (the last dimension contiguous); what has no
    such strides is copied."""
    _need_dtype(logits)
    if labels.dtype not in _ID_DT:
        raise ValueError(f"labels must be int32 or int64, got {labels.dtype}")
    if logits.dim() < 1 or tuple(labels.shape) != tuple(logits.shape[:-1]):
        raise ValueError(f"labels {tuple(labels.shape)} must have the logits' leading dimensions {tuple(logits.shape[:-1])}")
    V = logits.shape[-1]
    x = logits.detach()
    y = labels.detach()
    if x.dim() == 1:
        x, y = x[None, None], y[None, None]
    elif x.dim() == 2:
        x, y = x[None], y[None]
    elif x.dim() > 3:
        x, y = x.reshape(-1, x.shape[-2], V), y.reshape(-1, y.shape[-1])
    if V > 1 and x.stride(2) != 1:
        x = x.contiguous()
    return x, y


def _xent_desc(x: torch.Tensor, y: torch.Tensor, dx: Optional[torch.Tensor], ignore_index: int, label_smoothing: float, mean_reduction: bool = False):
    d = _lib.oeh_xent_desc()
    d.B, d.S, d.V, d.dtype = x.shape[0], x.shape[1], x.shape[2], _DT[x.dtype]
    d.label_dtype, d.mean_reduction = _ID_DT[y.dtype], int(bool(mean_reduction))
    d.x_stride[0], d.x_stride[1] = x.stride(0), x.stride(1)
    d.label_stride[0], d.label_stride[1] = y.stride(0), y.stride(1)
    if dx is not None:
        d.dx_stride[0], d.dx_stride[1] = dx.stride(0), dx.stride(1)
    d.ignore_index, d.label_smoothing = int(ignore_index), float(label_smoothing)
    return d


def xent_fwd(logits: torch.Tensor, labels: torch.Tensor, *, ignore_index: int = -100, label_smoothing: float = 0.0, want_rows: bool = False,
             meter: Optional[torch.Tensor] = None, bad_rows: Optional[torch.Tensor] = None):
    """Cross-entropy of `logits` (..., V) against integer `labels` (...) in one pass over the logits, which may be any view with a
    contiguous last dimension (`include/oeh.h: oeh_xent_fwd`).  Returns (mean, out2, lse, row_loss | None): the fp32 mean over the rows
    whose label is not `ignore_index` (NaN without one), a float64 {sum, count}, the rows' fp32 logsumexp and (want_rows, or with label
    smoothing) their fp32 losses, both flat.  meter: float64[2] on the same GPU, {sum of the means, calls}; bad_rows: int32[1] that counts
    the rows whose label is neither a class nor ignore_index (their loss is NaN).  Nothing synchronises."""
    global XENT_CALLS
    dev = _need_gpu(logits, labels, meter, bad_rows)
    x, y = _xent_views(logits, labels)
    rows = x.shape[0] * x.shape[1]
    if meter is not None:
        _need_f64(meter, 2, "meter must be a contiguous float64 tensor of 2 elements")
    if bad_rows is not None and (bad_rows.dtype != torch.int32 or bad_rows.numel() != 1):
        raise ValueError("bad_rows must be one int32")
    lse = torch.empty(rows, dtype=torch.float32, device=x.device)
    row_loss = torch.empty(rows, dtype=torch.float32, device=x.device) if want_rows or label_smoothing > 0.0 else None
    out2 = torch.empty(2, dtype=torch.float64, device=x.device)
    mean = torch.empty((), dtype=torch.float32, device=x.device)
    d = _xent_desc(x, y, None, ignore_index, label_smoothing)
    one = C.c_void_p(x.element_size() * 8)  # (an empty tensor has no address to hand over; nothing is read through this one)
    with _on_device(dev):
        rc = _lib.load().oeh_xent_fwd(C.byref(d), _ptr(x) if rows else one, _ptr(y) if rows else one, _ptr(lse) if rows else one,
                                      _ptr(row_loss) if rows or row_loss is None else one, _ptr(out2), _ptr(mean), _ptr(meter), _ptr(bad_rows), _stream())
    _lib.check(rc, "oeh_xent_fwd")
    XENT_CALLS += 1
    return mean, out2, lse, row_loss


def xent_bwd(logits: torch.Tensor, labels: torch.Tensor, lse: torch.Tensor, out2: torch.Tensor, grad: torch.Tensor, *, ignore_index: int = -100,
             label_smoothing: float = 0.0, mean_reduction: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The logit gradient of `xent_fwd` in one read and one write (`include/oeh.h: oeh_xent_bwd`): (softmax - smoothed one-hot) * g per
    row, g = `grad` - one fp32 value on the device, or one per row - divided by the forward's count with mean_reduction.  lse, out2: the
    forward's.  out: where to write, a tensor of the logits' shape and dtype with a contiguous last dimension; it may be `logits` itself."""
    dev = _need_gpu(logits, labels, lse, out2, grad, out)
    x, y = _xent_views(logits, labels)
    rows = x.shape[0] * x.shape[1]
    _need_f64(out2, 2, "out2 must be the forward's float64 {sum, count}")
    if lse.dtype != torch.float32 or lse.numel() != rows or not lse.is_contiguous():
        raise ValueError("lse must be the forward's: one contiguous fp32 value per row")
    g = grad.detach()
    if g.dtype != torch.float32 or g.numel() not in (1, rows) or not g.is_contiguous():
        raise ValueError("grad must be a contiguous fp32 tensor of one element, or of one per row")
    if out is None:
        out = torch.empty(logits.shape, dtype=logits.dtype, device=logits.device)
    elif tuple(out.shape) != tuple(logits.shape) or out.dtype != logits.dtype:
        raise ValueError("out must have the logits' shape and dtype")
    dx = out.detach()
    dx = dx[None, None] if dx.dim() == 1 else dx[None] if dx.dim() == 2 else dx
    if dx.dim() > 3:
        try:
            dx = dx.view(-1, dx.shape[-2], dx.shape[-1])  # (a view or nothing: the result must land in `out`)
        except RuntimeError:
            raise ValueError("out of more than three dimensions needs leading dimensions that fold into one") from None
    if tuple(dx.shape) != tuple(x.shape) or (x.shape[2] > 1 and dx.stride(2) != 1):
        raise ValueError("out needs a contiguous last dimension")
    if rows:
        d = _xent_desc(x, y, dx, ignore_index, label_smoothing, mean_reduction)
        with _on_device(dev):
            rc = _lib.load().oeh_xent_bwd(C.byref(d), _ptr(x), _ptr(y), _ptr(lse), _ptr(out2), _ptr(g), 0 if g.numel() == 1 else 1, _ptr(dx), _stream())
        _lib.check(rc, "oeh_xent_bwd")
    return out


def xent_variant(B: int, S: int, V: int, dtype=torch.float16, *, label_smoothing: float = 0.0, row_stride: Optional[int] = None, offset: int = 0,
                 dx_row_stride: Optional[int] = None, dx_offset: Optional[int] = None) -> Optional[str]:
    """Name of the launch form for (B, S, V) logits of `dtype` whose rows are `row_stride` (default V) elements apart and start `offset`
    elements behind a 16-byte boundary ("xent/block/CH4/f16", ".../ls" with smoothing), or None if refused.  With dx_offset (and
    dx_row_stride) the backward's form for a gradient tensor placed like that: ".../el" when its rows take element stores.  Host only."""
    if dtype not in _DT:
        return None
    eb = 4 if dtype == torch.float32 else 2
    st = V if row_stride is None else int(row_stride)
    d = _lib.oeh_xent_desc()
    d.B, d.S, d.V, d.dtype, d.label_dtype = int(B), int(S), int(V), _DT[dtype], _lib.OEH_ID_I64
    d.x_stride[0], d.x_stride[1] = st * int(S), st
    d.label_stride[0], d.label_stride[1] = int(S), 1
    d.label_smoothing = float(label_smoothing)
    dxp = None
    if dx_offset is not None:
        dst = V if dx_row_stride is None else int(dx_row_stride)
        d.dx_stride[0], d.dx_stride[1] = dst * int(S), dst
        dxp = C.c_void_p((1 << 20) + int(dx_offset) * eb)
    r = _lib.load().oeh_xent_variant(C.byref(d), C.c_void_p(4096 + int(offset) * eb), dxp)
    return None if r is None else r.decode()


# ---- the optimizer phase (include/oeh.h: oeh_mt_plan, oeh_grad_norm, oeh_grad_scale, oeh_adamw_step): one plan over all parameter tensors
MT_CHUNK = _lib.MT_CHUNK            # elements of one tensor that one workgroup covers
MT_MAX_GROUPS = _lib.MT_MAX_GROUPS  # hyper-parameter groups of one step
_grad_norm_work = {}  # (device index, stream handle) -> the per-chunk float64 partials of that stream's norm


@dataclass(frozen=True)
class AdamWGroup:
    """The hyper-parameters one kernel group is stepped with; `step` is the step number AFTER the increment (torch's)."""
    lr: float
    beta1: float
    beta2: float
    eps: float
    weight_decay: float
    step: int


class MtPlan:
    """The device table of a tensor list (`mt_plan`): the chunk entries and tensor records the multi-tensor kernels read, the number of
    chunks, and the tensors themselves - the table holds their addresses, so the plan keeps them alive (`hold_grads=False`: all but the
    gradients, whose addresses the caller then checks before every use).  `staging` is the pinned host copy the table was sent from."""

    def __init__(self, table, n_chunks, tensors, device, groups, numel, norm_only, records, staging):
        self.table, self.n_chunks, self.tensors, self.device = table, n_chunks, tensors, device
        self.groups, self.numel, self.norm_only, self._records, self.staging = groups, numel, norm_only, records, staging
        self.stream = None  # the raw handle of the stream the table was copied on

    @property
    def variants(self):
        """The access form of every non-empty tensor, in order: "vec16" or "elem" (include/oeh.h: oeh_mt_variant)."""
        lib = _lib.load()
        return [lib.oeh_mt_variant(C.byref(a)).decode() for a in self._records]


def mt_plan(params, grads, exp_avgs=None, exp_avg_sqs=None, groups=None, *, hold_grads: bool = True, replace: Optional[MtPlan] = None) -> MtPlan:
    """Plan the multi-tensor kernels over parallel lists: fp32 contiguous `params`, `exp_avgs`, `exp_avg_sqs`, and `grads` in fp32, fp16
    or bf16, all of a tensor's four with the same number of elements and everything on one GPU; groups[i] in [0, MT_MAX_GROUPS) says which
    `AdamWGroup` of `adamw_step` tensor i is stepped with (default 0).  With exp_avgs and exp_avg_sqs None the plan serves `grad_norm` and
    `grad_scale_` only (`params` may then be None as well).  hold_grads=False: the plan does not keep the gradients alive - for a caller who
    caches the plan across `zero_grad(set_to_none=True)` and compares every `data_ptr` before using it again (`optim.FusedAdamW`); a plan
    whose gradients were freed must not be launched.  replace: a plan of the caller's that is given up for this one - its device table is
    written over in place where it has the size (on the stream it was made on), so that planning again allocates nothing on the device
    and the allocator's picture stays as the training loop left it.  Host work and one small copy to the device, from pinned memory and in stream order:
    nothing waits for the device.  Reuse the plan while no tensor moves."""
    grads = list(grads)
    n = len(grads)
    norm_only = exp_avgs is None and exp_avg_sqs is None
    if norm_only:
        params = exp_avgs = exp_avg_sqs = [None] * n
    elif params is None or exp_avgs is None or exp_avg_sqs is None:
        raise ValueError("mt_plan needs params, exp_avgs and exp_avg_sqs together")
    params, exp_avgs, exp_avg_sqs = list(params), list(exp_avgs), list(exp_avg_sqs)
    groups = [0] * n if groups is None else [int(g) for g in groups]
    if not (len(params) == len(exp_avgs) == len(exp_avg_sqs) == len(groups) == n):
        raise ValueError("mt_plan needs lists of one length")
    dev = _need_gpu(*grads, *params, *exp_avgs, *exp_avg_sqs, allow_grad=True)
    keep, rows = [], []
    for p, g, m, v, grp in zip(params, grads, exp_avgs, exp_avg_sqs, groups):
        g = g.detach()
        if g.dtype not in _DT or g.is_sparse or not g.is_contiguous():
            raise ValueError("gradients must be dense contiguous fp32, fp16 or bf16 tensors")
        if not 0 <= grp < MT_MAX_GROUPS:
            raise ValueError(f"group {grp} outside [0, {MT_MAX_GROUPS})")
        if norm_only:
            p = m = v = None
        else:
            p, m, v = p.detach(), m.detach(), v.detach()
            for t_, what in ((p, "parameters"), (m, "exp_avgs"), (v, "exp_avg_sqs")):
                if t_.dtype != torch.float32 or not t_.is_contiguous() or t_.numel() != g.numel():
                    raise ValueError(f"{what} must be contiguous fp32 tensors with as many elements as their gradients")
        keep.append((p, g if hold_grads else None, m, v))
        if g.numel():  # (an empty tensor has no address and no chunk)
            # a norm-only plan names no p, m, v: the 16-byte boundary below g stands in, so that g alone decides the access form
            rows.append(tuple(g.data_ptr() & ~15 if t_ is None else t_.data_ptr() for t_ in (p, m, v)) + (g.data_ptr(), g.numel(), _DT[g.dtype], grp))
    arr = (_lib.oeh_mt_tensor * max(len(rows), 1))()
    for a, (pp, mp, vp, gp, cnt, dt, grp) in zip(arr, rows):
        a.p, a.g, a.m, a.v, a.n, a.g_dtype, a.group = pp, gp, mp, vp, cnt, dt, grp
    lib = _lib.load()
    nbytes = int(lib.oeh_mt_plan_bytes(arr, len(rows)))
    if nbytes < 0:
        _lib.check(lib.oeh_mt_plan(arr, len(rows), None, C.byref(C.c_int64())), "oeh_mt_plan")
    # (pinned, so that the copy below is an asynchronous one in stream order: a pageable source makes torch wait for the stream, i.e. for
    # the whole backward in front of an optimizer step.  torch's pinned-memory cache hands the block out again only after that copy has run.)
    host = torch.empty(max(nbytes // 8, 1), dtype=torch.int64, pin_memory=dev is not None)
    n_chunks = C.c_int64()
    _lib.check(lib.oeh_mt_plan(arr, len(rows), C.c_void_p(host.data_ptr()), C.byref(n_chunks)), "oeh_mt_plan")
    table, stream = None, None
    if dev is not None:
        with _on_device(dev):
            stream = _stream().value
            if replace is not None and replace.table is not None and replace.device == dev and replace.stream == stream and replace.table.numel() == host.numel():
                table = replace.table  # (stream order: every launch that read the old contents is in front of this copy)
                table.copy_(host, non_blocking=True)
            else:
                table = host.to(dev, non_blocking=True)
    plan = MtPlan(table, int(n_chunks.value), keep, dev, groups, sum(r[4] for r in rows), norm_only, arr[:len(rows)], host)
    plan.stream = stream
    return plan


def grad_norm(plan: MtPlan, max_norm: Optional[float] = None, *, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(4,) float64 on the plan's GPU: {sum of squares, 2-norm, clip coefficient, 0} over every gradient of the plan, the squares exact and
    summed in float64 in a fixed order (`include/oeh.h: oeh_grad_norm`); coefficient = min(1, max_norm / (norm + 1e-6)), 1 for max_norm None,
    <= 0 or inf.  out: a (4,) float64 tensor on that GPU to write into instead of a new one.  Two launches, nothing synchronises."""
    if plan.device is None:
        raise _lib.OehError("outeffhop_amd ops need GPU tensors: the HIP library is the only implementation")
    lib = _lib.load()
    if out is not None:
        _need_gpu(out, plan.table)
        _need_f64(out, 4, "out must be a contiguous float64 tensor of 4 elements")
    out4 = out if out is not None else torch.empty(4, dtype=torch.float64, device=plan.device)
    work = _scratch(_grad_norm_work, plan.device, max(int(lib.oeh_grad_norm_work_bytes(plan.n_chunks)), 8))
    with _on_device(plan.device):
        rc = lib.oeh_grad_norm(_ptr(plan.table), plan.n_chunks, 0.0 if max_norm is None else float(max_norm), _ptr(work), _ptr(out4), _stream())
    _lib.check(rc, "oeh_grad_norm")
    return out4


def grad_scale_(plan: MtPlan, clip: torch.Tensor) -> None:
    """Every gradient of the plan times clip[2] in place, rounded to fp32 once and then to the gradient's storage type (`clip`: a `grad_norm` result)."""
    if plan.device is None:
        raise _lib.OehError("outeffhop_amd ops need GPU tensors: the HIP library is the only implementation")
    _need_gpu(clip, plan.table)
    _need_f64(clip, 4, "clip must be the (4,) float64 result of grad_norm")
    with _on_device(plan.device):
        rc = _lib.load().oeh_grad_scale(_ptr(plan.table), plan.n_chunks, _ptr(clip), _stream())
    _lib.check(rc, "oeh_grad_scale")


def adamw_step(plan: MtPlan, groups, clip: Optional[torch.Tensor] = None) -> None:
    """One AdamW step of every tensor of the plan in one launch (`include/oeh.h: oeh_adamw_step`): groups[i] is the `AdamWGroup` of the
    tensors planned with group i.  clip: a `grad_norm` result whose coefficient scales the gradients as they are read - they are not
    written.  step and lr are host values recorded with the launch: not for graph capture."""
    if plan.device is None:
        raise _lib.OehError("outeffhop_amd ops need GPU tensors: the HIP library is the only implementation")
    if plan.norm_only:
        raise ValueError("this plan was made without exp_avgs and exp_avg_sqs: it serves grad_norm and grad_scale_ only")
    groups = list(groups)
    if not 1 <= len(groups) <= MT_MAX_GROUPS:
        raise ValueError(f"adamw_step takes 1 to {MT_MAX_GROUPS} groups")
    if plan.groups and max(plan.groups) >= len(groups):
        raise ValueError("a tensor of the plan names a group that was not given")
    d = _lib.oeh_adamw_desc()
    d.n_groups = len(groups)
    for i, g in enumerate(groups):
        d.lr[i], d.beta1[i], d.beta2[i], d.eps[i], d.weight_decay[i], d.step[i] = g.lr, g.beta1, g.beta2, g.eps, g.weight_decay, int(g.step)
    if clip is not None:
        _need_gpu(clip, plan.table)
        _need_f64(clip, 4, "clip must be the (4,) float64 result of grad_norm")
    with _on_device(plan.device):
        rc = _lib.load().oeh_adamw_step(_ptr(plan.table), plan.n_chunks, C.byref(d), _ptr(clip), _stream())
    _lib.check(rc, "oeh_adamw_step")


# ---- the same phase under fp16 loss scaling (include/oeh.h: oeh_grad_norm_amp, oeh_adamw_step_amp, oeh_loss_scale_update)
_adamw_amp_work = {}  # (device index, stream handle) -> the {bc2, ss} pair per plan record of that stream's step


def _need_f32_scalar(t: Optional[torch.Tensor], what: str) -> None:
    if t is not None and (t.dtype != torch.float32 or t.numel() != 1):
        raise ValueError(f"{what} must be a float32 tensor of one element")


def grad_norm_amp(plan: MtPlan, max_norm: Optional[float] = None, *, grad_scale: Optional[torch.Tensor] = None, found_inf: Optional[torch.Tensor] = None,
                  found_acc: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """`grad_norm` for gradients that carry a loss scale (`include/oeh.h: oeh_grad_norm_amp`): (4,) float64 {sum of squares of the gradients
    as stored, norm / s, clip coefficient / s, 1 if the step must be skipped else 0}.  grad_scale (s), found_inf and found_acc are
    one-element float32 tensors on the plan's GPU, each optional: the step is skipped when the sum is not finite, when found_inf is not 0 or
    when s is not a positive finite number; found_acc is then set to 1 and left alone otherwise.  Two launches, nothing synchronises."""
    if plan.device is None:
        raise _lib.OehError("outeffhop_amd ops need GPU tensors: the HIP library is the only implementation")
    lib = _lib.load()
    _need_gpu(grad_scale, found_inf, found_acc, out, plan.table)
    for t_, what in ((grad_scale, "grad_scale"), (found_inf, "found_inf"), (found_acc, "found_acc")):
        _need_f32_scalar(t_, what)
    if out is not None:
        _need_f64(out, 4, "out must be a contiguous float64 tensor of 4 elements")
    out4 = out if out is not None else torch.empty(4, dtype=torch.float64, device=plan.device)
    work = _scratch(_grad_norm_work, plan.device, max(int(lib.oeh_grad_norm_work_bytes(plan.n_chunks)), 8))
    with _on_device(plan.device):
        rc = lib.oeh_grad_norm_amp(_ptr(plan.table), plan.n_chunks, 0.0 if max_norm is None else float(max_norm), _ptr(grad_scale), _ptr(found_inf),
                                   _ptr(found_acc), _ptr(work), _ptr(out4), _stream())
    _lib.check(rc, "oeh_grad_norm_amp")
    return out4


class MtSlots:
    """Which device step counter each record of a plan advances (`mt_slots`): the int32 table on the device, the pinned copy it was sent
    from, and the entries as a tuple."""

    def __init__(self, table, staging, entries):
        self.table, self.staging, self.entries = table, staging, entries


def mt_slots(plan: MtPlan, slots, *, replace: Optional[MtSlots] = None) -> MtSlots:
    """The slot table of `adamw_step_amp` for `plan`: slots[i] is the index into `steps` of the plan's i-th non-empty tensor.  Entries must
    be distinct (two records that shared a counter would advance it twice; the device cannot tell) and as many as the plan has records.
    One small copy from pinned memory in stream order; replace: a table of the caller's to write over in place where it has the size."""
    entries = tuple(int(s) for s in slots)
    if plan.device is None:
        raise _lib.OehError("outeffhop_amd ops need GPU tensors: the HIP library is the only implementation")
    if len(entries) != len(plan._records):
        raise ValueError(f"the plan has {len(plan._records)} records, got {len(entries)} slots")
    if len(set(entries)) != len(entries) or any(not 0 <= s < 2 ** 31 for s in entries):
        raise ValueError("slots must be distinct indices: two records must not share a step counter")
    host = torch.empty(max(len(entries), 1), dtype=torch.int32, pin_memory=True)
    host[:len(entries)] = torch.tensor(entries, dtype=torch.int32)
    with _on_device(plan.device):
        if replace is not None and replace.table.device == plan.device and replace.table.numel() == host.numel():
            table = replace.table
            table.copy_(host, non_blocking=True)
        else:
            table = host.to(plan.device, non_blocking=True)
    return MtSlots(table, host, entries)


def adamw_step_amp(plan: MtPlan, groups, clip: torch.Tensor, steps: torch.Tensor, slots) -> torch.Tensor:
    """One AdamW step of every tensor of the plan under loss scaling (`include/oeh.h: oeh_adamw_step_amp`), two launches.  groups: as for
    `adamw_step`, their `step` ignored - the counters are `steps`, a contiguous float32 tensor on the plan's GPU, and record i advances
    steps[slots[i]] (`slots`: an `MtSlots` of this plan, or the indices themselves).  clip: a `grad_norm_amp` result; when its flag is set
    nothing is read or written - parameters, moments and counters stay.  Returns the (records, 2) float32 table {sqrt(1 - beta2^t),
    lr / (1 - beta1^t)} the step used: the stream's scratch, written again by the next call.  Nothing synchronises."""
    if plan.device is None:
        raise _lib.OehError("outeffhop_amd ops need GPU tensors: the HIP library is the only implementation")
    if plan.norm_only:
        raise ValueError("this plan was made without exp_avgs and exp_avg_sqs: it serves grad_norm and grad_scale_ only")
    groups = list(groups)
    if not 1 <= len(groups) <= MT_MAX_GROUPS:
        raise ValueError(f"adamw_step_amp takes 1 to {MT_MAX_GROUPS} groups")
    if plan.groups and max(plan.groups) >= len(groups):
        raise ValueError("a tensor of the plan names a group that was not given")
    if not isinstance(slots, MtSlots):
        slots = mt_slots(plan, slots)
    n = len(plan._records)
    if len(slots.entries) != n:
        raise ValueError(f"the plan has {n} records, the slot table {len(slots.entries)} entries")
    _need_gpu(clip, steps, slots.table, plan.table)
    _need_f64(clip, 4, "clip must be the (4,) float64 result of grad_norm_amp")
    if steps.dtype != torch.float32 or not steps.is_contiguous():
        raise ValueError("steps must be a contiguous float32 tensor")
    if slots.entries and max(slots.entries) >= steps.numel():
        raise ValueError(f"slot {max(slots.entries)} is outside the {steps.numel()} step counters")
    d = _lib.oeh_adamw_desc()
    d.n_groups = len(groups)
    for i, g in enumerate(groups):
        d.lr[i], d.beta1[i], d.beta2[i], d.eps[i], d.weight_decay[i] = g.lr, g.beta1, g.beta2, g.eps, g.weight_decay
    lib = _lib.load()
    work = _scratch(_adamw_amp_work, plan.device, max(int(lib.oeh_adamw_amp_work_bytes(n)), 8))
    with _on_device(plan.device):
        rc = lib.oeh_adamw_step_amp(_ptr(plan.table), plan.n_chunks, n, C.byref(d), _ptr(clip), _ptr(steps), _ptr(slots.table), _ptr(work), _stream())
    _lib.check(rc, "oeh_adamw_step_amp")
    return work.view(torch.float32)[:2 * n].view(n, 2)


def loss_scale_update(state: torch.Tensor, growth_factor: float, backoff_factor: float, growth_interval: int) -> None:
    """torch's _amp_update_scale_ rule on `state`, four float32 {scale, growth tracker, found, skipped} on a GPU, in one launch
    (`include/oeh.h: oeh_loss_scale_update`): back off and count the skip when found is set, grow after growth_interval clean steps
    (never to inf), then clear found."""
    dev = _need_gpu(state)
    if state.dtype != torch.float32 or state.numel() != 4 or not state.is_contiguous():
        raise ValueError("state must be a contiguous float32 tensor of 4 elements")
    with _on_device(dev):
        rc = _lib.load().oeh_loss_scale_update(_ptr(state), float(growth_factor), float(backoff_factor), int(growth_interval), _stream())
    _lib.check(rc, "oeh_loss_scale_update")


_calib_work = {}  # (device index, stream handle) -> the 36-KB histograms of that stream's on-device percentile selection


def percentile_ema(x: torch.Tensor, q_lo: float, q_hi: float, state: torch.Tensor, momentum: float = 0.9, first: bool = False) -> torch.Tensor:
    """(np.percentile(x, q_lo), np.percentile(x, q_hi)) blended into `state` (float64[2] on x's GPU) with the running average of
    RunningMinMaxEstimator (range_estimators.py:101-104), without leaving the device: `include/oeh.h: oeh_percentile_ema`."""
    dev = _need_gpu(x, state)
    _need_dtype(x)
    _need_f64(state, 2, "state must be a contiguous float64 tensor of 2 elements")
    xc = x.detach().contiguous()
    work = _scratch(_calib_work, dev, _lib.CALIB_WORK_BYTES)
    with _on_device(dev):
        rc = _lib.load().oeh_percentile_ema(_ptr(xc), xc.numel(), _DT[x.dtype], float(q_lo), float(q_hi), float(momentum), int(bool(first)),
                                            _ptr(state), _ptr(work), _stream())
    _lib.check(rc, "oeh_percentile_ema")
    return state


CALIB_SCORES, CALIB_PROBS, CALIB_CONTEXT = 0, 1, 2


def attn_calibrate(q: torch.Tensor, k: torch.Tensor, v: Optional[torch.Tensor], which: int, *, softmax: SoftmaxSpec = SoftmaxSpec(), scale: float = 1.0,
                   scale_div: float = 0.0, key_pad_mask: Optional[torch.Tensor] = None, full_mask: Optional[torch.Tensor] = None, causal: bool = False,
                   clamp_min: bool = False, mask_min: Optional[float] = None, scores_range: Optional[torch.Tensor] = None,
                   probs_range: Optional[torch.Tensor] = None, n_bits: int = 8, eps: float = 1e-8, q_lo: float = 0.001, q_hi: float = 99.999,
                   momentum: float = 0.9, first: bool = False, state: Optional[torch.Tensor] = None) -> Optional[torch.Tensor]:
    """Range estimation of the attention quantisers without the (B,H,Sq,Sk) tensors (`include/oeh.h: oeh_attn_calibrate`).
    which CALIB_SCORES / CALIB_PROBS: the percentile pair [+ running average] of the scaled scores / of the probabilities goes into
    `state` (float64[2] on the device), returned; CALIB_CONTEXT: returns the fp32 context, logical (B,H,Sq,D), stored (B,Sq,H,D).
    `scores_range` / `probs_range`: float64[2] device tensors (x_min, x_max) whose grids quantise the scores / probabilities on the
    way (None: not quantised)."""
    dev = _need_gpu(q, k, v, key_pad_mask, full_mask, scores_range, probs_range, state)
    B, H, Sq, D = q.shape
    Sk = k.shape[2]
    if k.shape != (B, H, Sk, D) or (v is not None and v.shape != (B, H, Sk, D)):
        raise ValueError("shape mismatch")
    if q.dtype not in _DT or k.dtype != q.dtype or (v is not None and v.dtype != q.dtype):
        raise ValueError("q / k / v dtypes must match and be fp16 / bf16 / fp32")
    fix = lambda t: t if t is None or t.stride(3) == 1 else t.contiguous()  # noqa: E731
    q, k, v = fix(q), fix(k), fix(v)
    out = None
    if which == CALIB_CONTEXT:
        out = torch.empty((B, Sq, H, D), dtype=torch.float32, device=q.device).permute(0, 2, 1, 3)
    # The statistics passes have no v (scores) and no output: the stride triples of the absent tensors are k's and q's.  o_dtype stays 0:
    # the context is fp32 whatever the storage, and the entry point does not read the field.
    d = _attn_desc(q, k, v if v is not None else k, out if out is not None else q, _DT[q.dtype], 0, softmax, scale, scale_div, causal, clamp_min,
                   mask_min, q.dtype)
    keep = []
    if key_pad_mask is not None:
        _set_key_pad(d, keep, key_pad_mask)  # (key_pad_boolean stays 0: this entry point has no such argument)
    if full_mask is not None:
        _set_full_mask(d, keep, full_mask)
    for r_ in (scores_range, probs_range, state):
        if r_ is not None:
            _need_f64(r_, 2, "ranges / state must be contiguous float64 tensors of 2 elements")
    work = None
    if which != CALIB_CONTEXT:
        if state is None:
            raise ValueError("state (float64[2] on the device) is required for the statistics passes")
        work = _scratch(_calib_work, dev, _lib.CALIB_WORK_BYTES)
    with _on_device(dev):
        rc = _lib.load().oeh_attn_calibrate(C.byref(d), _ptr(q), _ptr(k), _ptr(v), _ptr(out), int(which), _ptr(scores_range), _ptr(probs_range), int(n_bits),
                                            float(eps), float(q_lo), float(q_hi), float(momentum), int(bool(first)), _ptr(state), _ptr(work), _stream())
    _lib.check(rc, "oeh_attn_calibrate")
    return out if which == CALIB_CONTEXT else state


def fake_quant_range(x: torch.Tensor, xmin_xmax: torch.Tensor, n_bits: int = 8, eps: float = 1e-8) -> torch.Tensor:
    """Fake-quant with the grid derived on the device from a float64 (x_min, x_max) pair (`oeh_fake_quant_range`): the
    quantiser's forward while its range is still being estimated, without a host read of the range."""
    dev = _need_gpu(x, xmin_xmax)
    _need_dtype(x)
    _need_f64(xmin_xmax, 2, "xmin_xmax must be a contiguous float64 tensor of 2 elements")
    xc = x.contiguous()
    y = torch.empty_like(xc)
    with _on_device(dev):
        rc = _lib.load().oeh_fake_quant_range(_ptr(xc), _ptr(y), xc.numel(), _DT[x.dtype], _ptr(xmin_xmax), int(n_bits), float(eps), _stream())
    _lib.check(rc, "oeh_fake_quant_range")
    return y


def gate_fwd(hidden: torch.Tensor, H: int, w1: torch.Tensor, b1: torch.Tensor, w2: Optional[torch.Tensor] = None,
             b2: Optional[torch.Tensor] = None, per_head_pool: bool = False, scaling: float = 1.0) -> torch.Tensor:
    """Per-head gate predictors on the module input (bert_attention.py:301-327).  hidden (B,T,H*d);
    w1 (H,d)|(H,m,d), b1 (H)|(H,m), w2 (H,m), b2 (H).  Returns sigmoid(logit)*scaling as (B,H,T,1) or (B,H,1,1) fp32."""
    dev = _need_gpu(hidden, w1, b1, w2, b2)
    B, T, E = hidden.shape
    d = E // H
    hc = hidden if hidden.stride(2) == 1 else hidden.contiguous()
    m_units = 0 if w1.dim() == 2 else w1.shape[1]
    f = lambda t: None if t is None else t.detach().to(torch.float32).contiguous()  # noqa: E731
    w1, b1, w2, b2 = f(w1), f(b1), f(w2), f(b2)
    out = torch.empty((B, H, T), dtype=torch.float32, device=hidden.device)
    with _on_device(dev):
        rc = _lib.load().oeh_gate_fwd(_ptr(hc), _DT[hidden.dtype], B, T, H, d, hc.stride(0), hc.stride(1), _ptr(w1), _ptr(b1), _ptr(w2),
                                      _ptr(b2), m_units, int(per_head_pool), float(scaling), _ptr(out), _stream())
    _lib.check(rc, "oeh_gate_fwd")
    return out[:, :, :1, None] if per_head_pool else out[..., None]


def minmax(x: torch.Tensor) -> torch.Tensor:
    """(min, max) of a tensor as a 2-element fp32 GPU tensor, no host round trip (range_estimators.py:96-97)."""
    dev = _need_gpu(x)
    xc = x.contiguous()
    out = torch.empty(2, dtype=torch.float32, device=x.device)
    with _on_device(dev):
        rc = _lib.load().oeh_minmax(_ptr(xc), xc.numel(), _DT[x.dtype], _ptr(out), _stream())
    _lib.check(rc, "oeh_minmax")
    return out


# ---- outlier statistics (include/oeh.h: oeh_outlier_stats): the reference's two result metrics, per sample, in one pass

STATS_WAVE_COLS = _lib.STATS_WAVE_COLS  # W: rows up to this length take the one-wave, one-launch form (no work buffer)
STATS_CHUNK = _lib.STATS_CHUNK          # C: elements per (row, chunk) workgroup of the long-row form
STATS_INF_NORM, STATS_KURTOSIS, STATS_MEAN, STATS_STD = 0, 1, 2, 3  # columns of the result
_stats_work = {}  # (device index, stream handle) -> the chunk records of that stream


def outlier_stats(x: torch.Tensor, eps: float = 1e-6, meter: Optional[torch.Tensor] = None, accumulate: int = 0, *,
                  out: Optional[torch.Tensor] = None, work: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Per-sample (inf_norm, kurtosis, mean, std) of `x` viewed as (x.shape[0], -1): a (rows, 4) fp32 tensor from one pass over the
    data, no host synchronisation (`include/oeh.h: oeh_outlier_stats`; validate_clm.py:565-586 with transformers_language/utils.py:9-20).
    A view whose rows are dense and a row stride apart is read in place; anything else is made contiguous.  meter: float64[4] on x's
    GPU, {sum_inf, n_inf, sum_kurt, n_kurt}; accumulate: 1 adds this call's inf-norms, 2 its kurtoses, 3 both.  out / work: caller's
    buffers (tests); by default the result is new and the chunk records live in one buffer per stream."""
    dev = _need_gpu(x, meter, out, work)
    _need_dtype(x)
    if x.dim() < 2:
        raise ValueError("outlier_stats needs at least 2 dimensions: (samples, ...)")
    x = x.detach()
    rows = x.shape[0]
    cols = x.numel() // rows if rows else 0
    if not (rows >= 1 and cols >= 1 and (x[0].is_contiguous() or cols == 1) and (rows == 1 or x.stride(0) >= cols)):
        x = x.contiguous()
    row_stride = x.stride(0) if rows > 1 else cols
    if meter is not None:
        _need_f64(meter, 4, "meter must be a contiguous float64 tensor of 4 elements")
    if out is None:
        out = torch.empty((rows, 4), dtype=torch.float32, device=x.device)
    elif out.dtype != torch.float32 or tuple(out.shape) != (rows, 4) or not out.is_contiguous():
        raise ValueError("out must be a contiguous float32 tensor of shape (rows, 4)")
    lib = _lib.load()
    nbytes = lib.oeh_outlier_stats_work_bytes(rows, cols)
    if work is None:
        work = _scratch(_stats_work, dev, nbytes) if nbytes else None
    elif work.numel() * work.element_size() < nbytes:
        raise ValueError(f"work holds {work.numel() * work.element_size()} bytes, the call needs {nbytes}")
    with _on_device(dev):
        rc = lib.oeh_outlier_stats(_ptr(x), rows, cols, row_stride, _DT[x.dtype], float(eps), _ptr(out), _ptr(meter), int(accumulate), _ptr(work), _stream())
    _lib.check(rc, "oeh_outlier_stats")
    return out


def kurtosis(x: torch.Tensor, eps: float = 1e-6) -> torch.Tensor:
    """x - (B, d).  The reference's `kurtosis` (transformers_language/utils.py:9-20): mean((x - mu)^4) / (std^4 + eps) per row, as a
    (B,) fp32 tensor.  Deviation: the result is fp32, from fp32 / float64 arithmetic, for fp16 and bf16 inputs too - the reference
    evaluates (x - mu) ** 4 in the input's type there, which overflows fp16 from |x - mu| = 16 on."""
    return outlier_stats(x, eps)[:, STATS_KURTOSIS]


def inf_norm(x: torch.Tensor) -> torch.Tensor:
    """x.view(B, -1).norm(dim=1, p=inf) (validate_clm.py:575) as a (B,) fp32 tensor - fp32 for 16-bit inputs as well (the value is exact
    in either type)."""
    return outlier_stats(x)[:, STATS_INF_NORM]


# ---- quantisation-error search (include/oeh.h: oeh_quant_mse): the loss of every candidate grid of the MSE range estimator, one read

QMSE_CHUNK = _lib.QMSE_CHUNK            # C: elements a workgroup keeps in registers
QMSE_SLICE = _lib.QMSE_SLICE            # candidates per pass over the data
QMSE_MAX_BLOCKS = _lib.QMSE_MAX_BLOCKS  # workgroups per pass: above C * this many elements a workgroup takes several chunks
QMSE_F64_K = _lib.QMSE_F64_K            # calls of at most this many candidates add in float64 from the first term
_qmse_work = {}  # (device index, stream handle) -> the per-workgroup sums of that stream


def quant_grid_candidates(scale, lo, hi) -> torch.Tensor:
    """The (K, 4) fp32 candidate table of `quant_mse` from per-candidate scale, lo = int_min - zero_point and hi = int_max - zero_point
    (tensors or sequences of equal length; include/oeh.h documents the record)."""
    scale = torch.as_tensor(scale, dtype=torch.float32).reshape(-1)
    lo = torch.as_tensor(lo, dtype=torch.float32, device=scale.device).reshape(-1)
    hi = torch.as_tensor(hi, dtype=torch.float32, device=scale.device).reshape(-1)
    return torch.stack([scale, lo, hi, torch.zeros_like(scale)], dim=1).contiguous()


def quant_mse(x: torch.Tensor, cand: torch.Tensor, loss: Optional[torch.Tensor] = None, accumulate: bool = False, *,
              work: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The squared quantisation error of `x` on each of K candidate grids, as float64[K] on x's GPU, from one read of the data per
    QMSE_SLICE candidates and without a host synchronisation (`include/oeh.h: oeh_quant_mse`; the loss_fx of range_estimators.py:134-142,
    for all candidates at once).  cand: (K, 4) fp32 rows (scale, int_min - zero_point, int_max - zero_point, 0): `quant_grid_candidates`.
    loss: float64[K] to store into, or with `accumulate` to add to (one float64 add per candidate); by default a new tensor (zeros
    under `accumulate`).  The terms are fp32, rounded as the reference's eager ops round them; the sum is float64 from the 33rd term on.
    Deviation: fp16 and bf16 elements are widened to fp32 first - the reference would square and sum in the storage type and overflow
    fp16.  A dense view is read in place (any starting element); anything else is made contiguous.  work: caller's scratch (tests)."""
    dev = _need_gpu(x, cand, loss, work)
    _need_dtype(x)
    if cand.dtype != torch.float32 or cand.dim() != 2 or cand.shape[1] != 4 or not cand.is_contiguous():
        raise ValueError("cand must be a contiguous float32 tensor of shape (K, 4)")
    K = cand.shape[0]
    x = x.detach()
    if not x.is_contiguous():
        x = x.contiguous()
    if loss is None:
        loss = (torch.zeros if accumulate else torch.empty)(K, dtype=torch.float64, device=x.device)
    else:
        _need_f64(loss, K, "loss must be a contiguous float64 tensor of K elements")
    lib = _lib.load()
    nbytes = lib.oeh_quant_mse_work_bytes(x.numel(), K)
    if work is None:
        work = _scratch(_qmse_work, dev, max(nbytes, 8))
    elif work.numel() * work.element_size() < nbytes:
        raise ValueError(f"work holds {work.numel() * work.element_size()} bytes, the call needs {nbytes}")
    with _on_device(dev):
        rc = lib.oeh_quant_mse(_ptr(x), x.numel(), _DT[x.dtype], _ptr(cand), K, _ptr(loss), int(bool(accumulate)), _ptr(work), _stream())
    _lib.check(rc, "oeh_quant_mse")
    return loss


# ---- training: the forward with its row statistic and the fused backward (include/oeh.h: oeh_attn_fwd_train / oeh_attn_bwd)
def _train_desc(q, k, v, o, softmax, scale, scale_div, key_pad_mask, full_mask, causal, clamp_min, mask_min):
    """Descriptor + the mask views it points into, for the training entry points (fp16 / bf16, D = 64; the library refuses the rest)."""
    _check_qkv(q, k, v)  # (the callers hand over what `_rows16` made of their inputs: unit head-dim strides, nothing to replace)
    d = _attn_desc(q, k, v, o, _DT[q.dtype], _DT[q.dtype], softmax, scale, scale_div, causal, clamp_min, mask_min, q.dtype)
    keep = []
    # the masks may be part of an autograd graph here (the entry points allow it): detached, the views below record nothing
    if key_pad_mask is not None:
        _set_key_pad(d, keep, key_pad_mask.detach())  # (key_pad_boolean stays 0: the training entry points have no such argument)
    if full_mask is not None:
        _set_full_mask(d, keep, full_mask.detach())
    return d, keep


def _rows16(t: torch.Tensor) -> torch.Tensor:
    """A (B,H,S,D) view the training kernels can read: unit head-dim stride and 16-byte aligned rows (else a contiguous copy)."""
    eb = t.element_size()
    if t.stride(3) == 1 and t.data_ptr() % 16 == 0 and all((t.stride(i) * eb) % 16 == 0 for i in range(3)):
        return t
    return t.contiguous()


def train_supported(q: torch.Tensor, softmax: SoftmaxSpec) -> bool:
    """What oeh_attn_fwd_train / oeh_attn_bwd take (include/oeh.h): fp16 / bf16 storage, head dim 64, a registry softmax."""
    return q.dtype in (torch.float16, torch.bfloat16) and q.dim() == 4 and q.shape[3] == 64 and softmax is not None


def _dropout(p, seed):
    """oeh_dropout of (dropout_p, dropout_seed), or None for p == 0 (the entry points without dropout).  The library validates p
    (outside [0, 1) or NaN: OEH_EINVAL); the seed is a uint64 and has to be given with p != 0."""
    p = float(p)
    if p == 0.0:
        return None
    if seed is None:
        raise ValueError("dropout_p != 0 needs a dropout_seed (uint64)")
    seed = int(seed)
    if not 0 <= seed < 2 ** 64:
        raise ValueError(f"dropout_seed must be a uint64, got {seed}")
    return oeh_dropout(p, 0, seed)


def attn_fwd_train(q, k, v, *, softmax: SoftmaxSpec = SoftmaxSpec(), scale: float = 1.0, scale_div: float = 0.0, key_pad_mask=None,
                   full_mask=None, causal: bool = False, clamp_min: bool = False, mask_min: Optional[float] = None, dropout_p: float = 0.0,
                   dropout_seed: Optional[int] = None):
    """The attention core's forward for training: (o, lse).  o is the logical (B,H,Sq,D) result stored (B,Sq,H,D)-contiguous as attn_fwd's;
    lse (B,H,Sq) fp32 is the row statistic the backward recomputes the probabilities from.  No autograd here (see `fused_attention`).
    dropout_p > 0: attention dropout inside the kernel (include/oeh.h: oeh_attn_fwd_train_dropout), its mask drawn from dropout_seed -
    the backward needs the same two values; lse does not depend on them."""
    dev = _need_gpu(q, k, v, key_pad_mask, full_mask, allow_grad=True)
    if q.dim() != 4 or k.dim() != 4 or v.dim() != 4:
        raise ValueError("q, k, v must be 4-D (B,H,S,D) views")
    q, k, v = _rows16(q.detach()), _rows16(k.detach()), _rows16(v.detach())
    B, H, Sq, D = q.shape
    o = torch.empty((B, Sq, H, D), dtype=q.dtype, device=q.device).permute(0, 2, 1, 3)
    lse = torch.empty((B, H, Sq), dtype=torch.float32, device=q.device)
    d, keep = _train_desc(q, k, v, o, softmax, scale, scale_div, key_pad_mask, full_mask, causal, clamp_min, mask_min)
    drop = _dropout(dropout_p, dropout_seed)
    lib = _lib.load()
    with _on_device(dev):
        if drop is None:
            rc = lib.oeh_attn_fwd_train(C.byref(d), _ptr(q), _ptr(k), _ptr(v), _ptr(o), _ptr(lse), _stream())
        else:
            rc = lib.oeh_attn_fwd_train_dropout(C.byref(d), C.byref(drop), _ptr(q), _ptr(k), _ptr(v), _ptr(o), _ptr(lse), _stream())
    _lib.check(rc, "oeh_attn_fwd_train" if drop is None else "oeh_attn_fwd_train_dropout")
    del keep
    return o, lse


def attn_bwd(q, k, v, o, do, lse, *, softmax: SoftmaxSpec = SoftmaxSpec(), scale: float = 1.0, scale_div: float = 0.0, key_pad_mask=None,
             full_mask=None, causal: bool = False, clamp_min: bool = False, mask_min: Optional[float] = None, dropout_p: float = 0.0,
             dropout_seed: Optional[int] = None):
    """(dq, dk, dv) of the attention core from the forward's o and lse (attn_fwd_train) and the output gradient do; same options as that
    call, dropout_p / dropout_seed included.  Two HIP kernels, deterministic (no atomics); the gradients are (B,S,H,D)-contiguous (B,H,S,D)
    views in the input dtype."""
    dev = _need_gpu(q, k, v, o, do, lse, key_pad_mask, full_mask, allow_grad=True)
    q, k, v, o, do = (_rows16(t.detach()) for t in (q, k, v, o, do))
    if do.shape != o.shape or do.dtype != o.dtype:
        do = _rows16(do.to(o.dtype))
    B, H, Sq, D = q.shape
    Sk = k.shape[2]
    if lse.shape != (B, H, Sq) or lse.dtype != torch.float32 or not lse.is_contiguous():
        raise ValueError("lse must be the contiguous fp32 (B,H,Sq) statistic of attn_fwd_train")
    new = lambda S: torch.empty((B, S, H, D), dtype=q.dtype, device=q.device).permute(0, 2, 1, 3)  # noqa: E731
    dq, dk, dv = new(Sq), new(Sk), new(Sk)
    d, keep = _train_desc(q, k, v, o, softmax, scale, scale_div, key_pad_mask, full_mask, causal, clamp_min, mask_min)
    lib = _lib.load()
    nbytes = lib.oeh_attn_bwd_work_bytes(C.byref(d))
    if nbytes < 0:
        _lib.check(int(nbytes), "oeh_attn_bwd_work_bytes")
    work = torch.empty((max(1, nbytes // 4),), dtype=torch.float32, device=q.device)
    st = lambda t: (C.c_int64 * 3)(t.stride(0), t.stride(1), t.stride(2))  # noqa: E731
    drop = _dropout(dropout_p, dropout_seed)
    with _on_device(dev):
        if drop is None:
            rc = lib.oeh_attn_bwd(C.byref(d), _ptr(q), _ptr(k), _ptr(v), _ptr(o), _ptr(do), st(do), _ptr(lse), _ptr(dq), st(dq), _ptr(dk), st(dk),
                                  _ptr(dv), st(dv), _ptr(work), _stream())
        else:
            rc = lib.oeh_attn_bwd_dropout(C.byref(d), C.byref(drop), _ptr(q), _ptr(k), _ptr(v), _ptr(o), _ptr(do), st(do), _ptr(lse), _ptr(dq),
                                          st(dq), _ptr(dk), st(dk), _ptr(dv), st(dv), _ptr(work), _stream())
    _lib.check(rc, "oeh_attn_bwd" if drop is None else "oeh_attn_bwd_dropout")
    del keep
    return dq, dk, dv


def attn_dropout_mask(B: int, H: int, Sq: int, Sk: int, p: float, seed: int, device) -> torch.Tensor:
    """The keep mask the training kernels apply for (p, seed): a (B,H,Sq,Sk) bool tensor on `device`, True where an attention
    probability is kept (and scaled by 1 / (1 - p)).  include/oeh.h: oeh_attn_dropout_mask; p == 0 keeps everything."""
    device = torch.device(device)
    if device.type != "cuda":
        raise _lib.OehError("outeffhop_amd ops need GPU tensors: the HIP library is the only implementation")
    d = oeh_attn_desc()
    d.B, d.H, d.Sq, d.Sk = int(B), int(H), int(Sq), int(Sk)
    p = float(p)
    drop = oeh_dropout(p, 0, int(seed) if seed is not None else 0) if p == 0.0 else _dropout(p, seed)
    keep = torch.empty((B, H, Sq, Sk), dtype=torch.uint8, device=device)
    lib = _lib.load()
    with _on_device(device):
        rc = lib.oeh_attn_dropout_mask(C.byref(d), C.byref(drop), _ptr(keep), _stream())
    _lib.check(rc, "oeh_attn_dropout_mask")
    return keep.view(torch.bool)


# ---- the softmax rows of the unfused path in training (include/oeh.h: oeh_softmax_train_fwd / oeh_softmax_train_bwd): scale + mask + clamp +
# softmax / softmax_1 + clip + dropout in one pass, and the backward from the scores and two fp32 numbers per row
SOFTMAX_TRAIN_MAX_COLS = _lib.SOFTMAX_TRAIN_MAX_COLS  # rows longer than this are refused (OEH_ENOTSUP)
SOFTMAX_TRAIN_CALLS = 0  # launches of `softmax_train_fwd` (softmax.FUSED_SOFTMAX_TRAIN)


def _st3(t: Optional[torch.Tensor], shape=None):
    """The (b, h, i) element strides of a 4-D tensor; with `shape`: of a tensor broadcast against it (0 where its own extent is 1)."""
    if t is None:
        return (0, 0, 0)
    return tuple(0 if (shape is not None and t.shape[k] == 1 and shape[k] != 1) else t.stride(k) for k in range(3))


def _softmax_train_desc(x, y_dtype, mask, spec: SoftmaxSpec, scale, scale_div, clamp_min, p, seed) -> _lib.oeh_softmax_train_desc:
    d = _lib.oeh_softmax_train_desc()
    d.B, d.H, d.Sq, d.Sk = x.shape
    d.x_dtype, d.y_dtype = _DT[x.dtype], _DT[y_dtype]
    d.mask_dtype = _DT[mask.dtype] if mask is not None else -1
    d.softmax_base, d.clip, d.gamma, d.eta = int(spec.base), int(bool(spec.clip)), float(spec.gamma), float(spec.eta)
    d.scale, d.scale_div = float(scale), float(scale_div)
    d.clamp, d.clamp_min = (0, 0.0) if clamp_min is None else (1, float(clamp_min))
    d.x_stride = _st3(x)
    d.mask_stride = _st3(mask, x.shape)
    drop = _dropout(p, seed)
    d.drop.p, d.drop.seed = (0.0, 0) if drop is None else (drop.p, drop.seed)
    return d


def _softmax_train_in(op: str, x, mask, y_dtype):
    if x.dim() != 4 or (x.shape[3] > 1 and x.stride(3) != 1):
        raise ValueError(f"{op} takes (B,H,Sq,Sk) scores whose last dimension is contiguous")
    _need_dtype(x)
    if y_dtype not in (x.dtype, torch.float32):
        raise ValueError(f"{op}: the output dtype is the scores' or float32")
    if mask is not None:
        if mask.dim() != 4 or mask.dtype not in _DT or mask.shape[3] != x.shape[3] or (mask.shape[3] > 1 and mask.stride(3) != 1) or \
                any(mask.shape[k] not in (1, x.shape[k]) for k in range(3)):
            raise ValueError(f"{op}: the additive mask is a 4-D fp16 / bf16 / fp32 tensor that broadcasts over (B,H,Sq) and has contiguous (Sk) rows")


def softmax_train_fwd(x: torch.Tensor, spec: SoftmaxSpec = SoftmaxSpec(), *, scale: float = 1.0, scale_div: float = 0.0, mask: Optional[torch.Tensor] = None,
                      clamp_min: Optional[float] = None, p: float = 0.0, seed: Optional[int] = None, out_dtype=None, want_y: bool = True):
    """(y, u, stats) of the softmax rows of (B,H,Sq,Sk) scores in ONE kernel (`include/oeh.h: oeh_softmax_train_fwd`): y = clip(softmax[_1](max(x * scale
    [or x / scale_div] + mask, clamp_min))) in `out_dtype` (x's, or float32), u = dropout(y) (None with p == 0; its keep mask is
    `attn_dropout_mask(B, H, Sq, Sk, p, seed)`), stats (B,H,Sq,2) fp32 = the row's maximum and denominator, what `softmax_train_bwd` reads.
    y is None without want_y (p > 0 only).  No autograd here (see `softmax.masked_softmax`)."""
    global SOFTMAX_TRAIN_CALLS
    dev = _need_gpu(x, mask, allow_grad=True)
    y_dtype = x.dtype if out_dtype is None else out_dtype
    x, mask = x.detach(), None if mask is None else mask.detach()
    _softmax_train_in("softmax_train_fwd", x, mask, y_dtype)
    d = _softmax_train_desc(x, y_dtype, mask, spec, scale, scale_div, clamp_min, p, seed)
    drop = d.drop.p > 0.0
    if not want_y and not drop:
        raise ValueError("softmax_train_fwd: nothing to compute (want_y=False without dropout)")
    y = torch.empty(x.shape, dtype=y_dtype, device=x.device) if want_y else None
    u = torch.empty(x.shape, dtype=y_dtype, device=x.device) if drop else None
    stats = torch.empty(tuple(x.shape[:3]) + (2,), dtype=torch.float32, device=x.device)
    d.y_stride, d.u_stride = _st3(y), _st3(u)
    if x.numel():  # (an empty tensor has no address to hand over)
        with _on_device(dev):
            rc = _lib.load().oeh_softmax_train_fwd(C.byref(d), _ptr(x), _ptr(mask), _ptr(y), _ptr(u), _ptr(stats), _stream())
        _lib.check(rc, "oeh_softmax_train_fwd")
        SOFTMAX_TRAIN_CALLS += 1
    return y, u, stats


def softmax_train_bwd(x: torch.Tensor, stats: torch.Tensor, dy: Optional[torch.Tensor], du: Optional[torch.Tensor], spec: SoftmaxSpec = SoftmaxSpec(), *,
                      scale: float = 1.0, scale_div: float = 0.0, mask: Optional[torch.Tensor] = None, clamp_min: Optional[float] = None, p: float = 0.0,
                      seed: Optional[int] = None) -> torch.Tensor:
    """dx of `softmax_train_fwd` from its scores, mask, stats and options and the gradients that arrived on y and / or u (either may be None;
    both have the forward's out_dtype).  One kernel, no atomics: the same bits on every call (`include/oeh.h: oeh_softmax_train_bwd`)."""
    dev = _need_gpu(x, mask, stats, dy, du, allow_grad=True)
    g = dy if dy is not None else du
    if g is None:
        raise ValueError("softmax_train_bwd needs dy or du")
    x, mask = x.detach(), None if mask is None else mask.detach()
    _softmax_train_in("softmax_train_bwd", x, mask, g.dtype)
    if stats.shape != tuple(x.shape[:3]) + (2,) or stats.dtype != torch.float32 or not stats.is_contiguous():
        raise ValueError("stats must be the contiguous fp32 (B,H,Sq,2) row statistic of softmax_train_fwd")
    grads = []
    for t_, what in ((dy, "dy"), (du, "du")):
        if t_ is not None:
            if t_.shape != x.shape or t_.dtype != g.dtype:
                raise ValueError(f"{what} must have the scores' shape and the forward's out_dtype")
            t_ = t_.detach()
            t_ = t_ if (t_.shape[3] == 1 or t_.stride(3) == 1) and all(s >= 0 for s in t_.stride()) else t_.contiguous()
        grads.append(t_)
    dy, du = grads
    d = _softmax_train_desc(x, g.dtype, mask, spec, scale, scale_div, clamp_min, p, seed)
    dx = torch.empty(x.shape, dtype=x.dtype, device=x.device)
    d.dy_stride, d.du_stride, d.dx_stride = _st3(dy), _st3(du), _st3(dx)
    if x.numel():
        with _on_device(dev):
            rc = _lib.load().oeh_softmax_train_bwd(C.byref(d), _ptr(x), _ptr(mask), _ptr(stats), _ptr(dy), _ptr(du), _ptr(dx), _stream())
        _lib.check(rc, "oeh_softmax_train_bwd")
    return dx


def softmax_train_variant(B: int, H: int, Sq: int, Sk: int, dtype=torch.float16, *, backward: bool = False, spec: SoftmaxSpec = SoftmaxSpec(),
                          out_dtype=None, mask_dtype=None, clamp: bool = False, p: float = 0.0, row_stride: Optional[int] = None) -> Optional[str]:
    """Name of the launch form the training softmax takes for contiguous (B,H,Sq,Sk) scores of `dtype` (rows `row_stride` elements apart,
    default Sk) with 16-byte aligned pointers: "softmax_train/fwd/lanes/G4x8/f16/softmax1", ".../wave/CH2/...", ".../block/...", or None
    if refused.  Host only."""
    d = _lib.oeh_softmax_train_desc()
    d.B, d.H, d.Sq, d.Sk = int(B), int(H), int(Sq), int(Sk)
    d.x_dtype = _DT[dtype]
    d.y_dtype = _DT[dtype if out_dtype is None else out_dtype]
    d.mask_dtype = -1 if mask_dtype is None else _DT[mask_dtype]
    d.softmax_base, d.clip, d.gamma, d.eta = int(spec.base), int(bool(spec.clip)), float(spec.gamma), float(spec.eta)
    d.scale, d.clamp = 1.0, int(bool(clamp))
    rs = int(Sk) if row_stride is None else int(row_stride)
    st = (H * Sq * rs, Sq * rs, rs)
    d.x_stride = d.y_stride = d.u_stride = d.mask_stride = d.dy_stride = d.du_stride = d.dx_stride = st
    d.drop.p = float(p)
    r = _lib.load().oeh_softmax_train_variant(C.byref(d), int(bool(backward)))
    return None if r is None else r.decode()


# ---- the per-token gate in training (include/oeh.h: oeh_gate_apply_fwd / oeh_gate_apply_bwd): predictors + sigmoid + context * gate, both directions
GATE_TRAIN_DIMS = (32, 64)   # head dims the kernels take (OEH_ENOTSUP otherwise)
GATE_TRAIN_MAX_UNITS = 64    # hidden units of an MLP predictor
_gate_train_work = {}  # (device index, stream handle) -> the per-workgroup parameter-gradient records of that stream's backward


def _gate_train_desc(B: int, T: int, H: int, d: int, units: int, dtype, scaling: float, hidden_stride, ctx_stride, out_stride,
                     dctx_stride=(0, 0, 0), dhidden_stride=(0, 0)) -> _lib.oeh_gate_train_desc:
    """hidden / out (dout) / dhidden: (batch, token) element strides; ctx / dctx: (batch, head, token).  The library validates the rest."""
    g = _lib.oeh_gate_train_desc()
    g.B, g.T, g.H, g.d, g.units, g.dtype = int(B), int(T), int(H), int(d), int(units), _DT[dtype]
    g.scaling = float(scaling)
    g.hidden_stride, g.ctx_stride, g.out_stride = tuple(hidden_stride), tuple(ctx_stride), tuple(out_stride)
    g.dctx_stride, g.dhidden_stride = tuple(dctx_stride), tuple(dhidden_stride)
    return g


def _gate_train_in(op: str, ctx: torch.Tensor, hidden: torch.Tensor, w1, b1, w2, b2):
    """Shapes of one gate call: ctx (B,H,T,d) and hidden (B,T,H*d) of one storage dtype with contiguous last dimensions, the stacked fp32
    predictor weights of `attention.GateState.packed_weights`.  Returns (B, H, T, d, units)."""
    _need_dtype(ctx)
    if ctx.dim() != 4 or hidden.dim() != 3 or hidden.dtype != ctx.dtype:
        raise ValueError(f"{op}: ctx (B,H,T,d) and hidden (B,T,H*d) of one dtype")
    B, H, T, d = ctx.shape
    if tuple(hidden.shape) != (B, T, H * d) or ctx.stride(3) != 1 or hidden.stride(2) != 1:
        raise ValueError(f"{op}: hidden must be (B,T,H*d) and both last dimensions contiguous")
    units = 0 if w1.dim() == 2 else int(w1.shape[1])
    shapes = ((w1, (H, d)), (b1, (H,))) if units == 0 else ((w1, (H, units, d)), (b1, (H, units)), (w2, (H, units)), (b2, (H,)))
    for w, shape in shapes:
        if w is None or tuple(w.shape) != shape or w.dtype != torch.float32 or not w.is_contiguous():
            raise ValueError(f"{op}: predictor weights must be the stacked contiguous fp32 arrays of oeh_gate_fwd, expected {shape}")
    return B, H, T, d, units


def gate_apply_fwd(ctx: torch.Tensor, hidden: torch.Tensor, w1: torch.Tensor, b1: torch.Tensor, w2: Optional[torch.Tensor] = None,
                   b2: Optional[torch.Tensor] = None, scaling: float = 1.0):
    """(out, gate_out) of the conditional per-token gate applied to a context (`include/oeh.h: oeh_gate_apply_fwd`): gate_out (B,H,T) fp32 =
    sigmoid(predictor_h(hidden[:, :, h d:(h + 1) d])) WITHOUT the scaling - the bits of `gate_fwd(..., scaling=1)` - and out (B,T,H*d) =
    ctx (B,H,T,d, any batch / head / token strides) * (gate_out * scaling) in ctx's dtype, heads merged.  w1 (H,d) | (H,m,d), b1 (H) | (H,m),
    w2 (H,m), b2 (H): contiguous fp32.  No autograd here (see `attention.GateApply`)."""
    dev = _need_gpu(ctx, hidden, w1, b1, w2, b2, allow_grad=True)
    B, H, T, d, units = _gate_train_in("gate_apply_fwd", ctx, hidden, w1, b1, w2, b2)
    ctx, hidden = ctx.detach(), hidden.detach()
    out = torch.empty((B, T, H * d), dtype=ctx.dtype, device=ctx.device)
    gate_out = torch.empty((B, H, T), dtype=torch.float32, device=ctx.device)
    g = _gate_train_desc(B, T, H, d, units, ctx.dtype, scaling, hidden.stride()[:2], ctx.stride()[:3], out.stride()[:2])
    with _on_device(dev):
        rc = _lib.load().oeh_gate_apply_fwd(C.byref(g), _ptr(hidden), _ptr(w1), _ptr(b1), _ptr(w2), _ptr(b2), _ptr(ctx), _ptr(gate_out), _ptr(out), _stream())
    _lib.check(rc, "oeh_gate_apply_fwd")
    return out, gate_out


def gate_apply_bwd(dout: torch.Tensor, ctx: torch.Tensor, hidden: torch.Tensor, gate_out: torch.Tensor, w1: torch.Tensor, b1: torch.Tensor,
                   w2: Optional[torch.Tensor] = None, b2: Optional[torch.Tensor] = None, scaling: float = 1.0, *, want_dhidden: bool = True,
                   dctx: Optional[torch.Tensor] = None, dhidden: Optional[torch.Tensor] = None):
    """(dctx, dhidden, dw1, db1, dw2, db2) of `gate_apply_fwd` from the output gradient dout (B,T,H*d), the forward's inputs and its gate_out
    (`include/oeh.h: oeh_gate_apply_bwd`).  dctx: contiguous (B,H,T,d) in ctx's dtype; dhidden: (B,T,H*d) (None without want_dhidden: the
    other outputs keep their bits); the parameter gradients: fp32 in the weights' stacked layouts (dw2, db2 None for a Linear predictor),
    summed in float64 and rounded once.  Nothing of the hidden layer is read: it is formed again from hidden.  Two HIP kernels, no atomics:
    the same bits on every call.  dctx / dhidden: the caller's output tensors of those shapes in ctx's dtype, any (batch, head, token) /
    (batch, token) strides with a contiguous last dimension and 16-byte aligned rows."""
    dev = _need_gpu(dout, ctx, hidden, gate_out, w1, b1, w2, b2, dctx, dhidden, allow_grad=True)
    B, H, T, d, units = _gate_train_in("gate_apply_bwd", ctx, hidden, w1, b1, w2, b2)
    if tuple(dout.shape) != (B, T, H * d) or dout.dtype != ctx.dtype:
        raise ValueError("gate_apply_bwd: dout must be (B,T,H*d) in ctx's dtype")
    if tuple(gate_out.shape) != (B, H, T) or gate_out.dtype != torch.float32 or not gate_out.is_contiguous():
        raise ValueError("gate_apply_bwd: gate_out must be the contiguous fp32 (B,H,T) tensor of gate_apply_fwd")
    dout = dout.detach()
    if dout.stride(2) != 1:
        dout = dout.contiguous()
    ctx, hidden = ctx.detach(), hidden.detach()
    for t_, shape, what in ((dctx, (B, H, T, d), "dctx"), (dhidden, (B, T, H * d), "dhidden")):
        if t_ is not None and (tuple(t_.shape) != shape or t_.dtype != ctx.dtype or t_.stride(-1) != 1):
            raise ValueError(f"gate_apply_bwd: {what} must be {shape} in ctx's dtype with a contiguous last dimension")
    if dctx is None:
        dctx = torch.empty((B, H, T, d), dtype=ctx.dtype, device=ctx.device)
    want_dhidden = want_dhidden or dhidden is not None
    if dhidden is None and want_dhidden:
        dhidden = torch.empty((B, T, H * d), dtype=ctx.dtype, device=ctx.device)
    dw1, db1 = torch.empty_like(w1), torch.empty_like(b1)
    dw2, db2 = (torch.empty_like(w2), torch.empty_like(b2)) if units > 0 else (None, None)
    g = _gate_train_desc(B, T, H, d, units, ctx.dtype, scaling, hidden.stride()[:2], ctx.stride()[:3], dout.stride()[:2], dctx.stride()[:3],
                         dhidden.stride()[:2] if want_dhidden else (0, 0))
    lib = _lib.load()
    nbytes = int(lib.oeh_gate_apply_bwd_work_bytes(B, T, H, d, units))
    _lib.check(min(nbytes, 0), "oeh_gate_apply_bwd_work_bytes")
    work = _scratch(_gate_train_work, dev, max(nbytes, 8))
    with _on_device(dev):
        rc = lib.oeh_gate_apply_bwd(C.byref(g), _ptr(dout), _ptr(ctx), _ptr(hidden), _ptr(gate_out), _ptr(w1), _ptr(b1), _ptr(w2), _ptr(b2), _ptr(dctx),
                                    _ptr(dhidden), _ptr(dw1), _ptr(db1), _ptr(dw2), _ptr(db2), _ptr(work), _stream())
    _lib.check(rc, "oeh_gate_apply_bwd")
    return dctx, dhidden, dw1, db1, dw2, db2


def gate_apply_variant(B: int, T: int, H: int, d: int, units: int = 0, dtype=torch.float16, *, backward: bool = False) -> Optional[str]:
    """Name of the launch form the training gate takes for contiguous tensors: "gate_train/fwd/D64/M16/f16", "gate_train/bwd/D64/M16/f16/G64x2"
    (backward: workgroups per head x 64-token tiles per workgroup), or None if refused.  Host only."""
    E = int(H) * int(d)
    g = _gate_train_desc(B, T, H, d, units, dtype, 1.0, (T * E, E), (T * E, T * d, d), (T * E, E), (T * E, T * d, d), (T * E, E))
    r = _lib.load().oeh_gate_apply_variant(C.byref(g), int(bool(backward)))
    return None if r is None else r.decode()
