"""Every kernel, K-loop form and epilogue branch of the projection GEMM (csrc/oeh_gemm.hip behind `oeh_proj_quant_i8`), each reached BY
SHAPE through the rules of `launch_gemm`, against EXACT arithmetic.  `-m gpu`.

The exact cases build operands for which every accumulation order gives the same accumulator: activations and weights are integer
multiples of one unit, sum |a| |w| / unit < 2^24 (asserted), alpha and the quantiser steps are powers of two and the bias lies on the
grid alpha * unit.  alpha * acc + bias and its quotient by the step are then exact in fp32, quotients land exactly on .5 ties and beyond
both ends of the grid, and indices and values are compared with `torch.equal` against float64 arithmetic and the reference's quantiser
formula clamp(round(v / scale) + zero_point, 0, 255) (uniform_quantizers.py:114-148; round = half to even).  The operand pairs and the
fp32 activations carry 14 significant bits (integers up to 31 + multiples of 2^-9): without the `lo` half - the second MFMA product,
the in-kernel v_fma_mix split - the sums are wrong.  Every output is an interior slice of a larger buffer filled with a sentinel, the
margins (and the pad columns of a value matrix with y_stride_row > E) must come back untouched; pad columns of `a` and `w` (lda, ldw >
K) hold NaN (int8: 127).

launch_gemm (t0 = ceil(M / 128) ceil(N / 288), waste = t0 128 288 / (M N); `form`: fp16 | pairs | fp32 | int8 = pairs 0 | 1 | 2 | 3):
    big   = t0 >= 512 and waste <= 1.06                              -> <form, 4, 9>  (fp32: <A_F32, 4, 9, LOOP = 2>)
    loop1 = fp32 and 160 <= t0 <= 256 and waste <= 1.06 and K >= 64  -> <A_F32, 4, 9, LOOP = 1>
    else                                                             -> <form, 2, 6>
Workgroup -> tile: MT % 8 == 0 the XCD map, else the linear one (MT = row tiles of the chosen tile).  K steps T = K / 32 (int8: K / 64).

case (test id)            M x N (E x segments)   kernel                        host condition                 what it adds
------------------------  ---------------------  ----------------------------  -----------------------------  ------------------------------------------
small[tail-*]             16 x 64 (64 x 1)       <fp16|pairs|fp32|int8, 2, 6>  t0 = 1 < 512                   one tile, mostly tail; T = 1; linear map (MT = 1)
small[ragged-*]           80 x 192 (64 x 3)      <.., 2, 6>                    t0 = 1                         ragged M (MT = 2), boundaries at columns 64, 128 of one tile, T = 2,
                                                                                                              transposed segment with S = 16 (a row tile spans 4 batch elements), lda, ldw > K
small[xcd-*]              512 x 384 (128 x 3)    <.., 2, 6>                    t0 = 8                         MT = 8: the XCD map; NT = 2; boundary at 128 inside tile 0, 256 inside tile 1; T = 3; values only
small[linear-*]           576 x 128 (64 x 2)     <.., 2, 6>                    t0 = 5                         MT = 9: linear map; ragged N; S = 48 transposed; y_stride_row > E (C ABI)
forms[*-rot0..4]          240 x 192 (64 x 3)     <.., 2, 6>                    t0 = 2                         values + row-major | values + transposed | values only | row-major only | transposed only,
                                                                                                              each in segment positions 0, 1, 2; zero points 0, 255, 117 rotate with them; S = 48
values_on_off[*]          80 x 192               <.., 2, 6>                    t0 = 1                         the fmed3 clamp (values) and v_cvt_pk_u8_f32's saturation (no values): equal indices
loop1[2560-K64]           2560 x 2304 (768 x 3)  <A_F32, 4, 9, 1>              t0 = 160, waste 1.0, K >= 64   T = 2: the ring's two-step tail alone; MT = 20: linear map
loop1[2576-K96]           2576 x 2304            <A_F32, 4, 9, 1>              t0 = 168, waste 1.043          ragged last row tile, MT = 21; T = 3: one full step + the tail
loop1[4096-K128]          4096 x 2304            <A_F32, 4, 9, 1>              t0 = 256                       MT = 32: the XCD map; T = 4: the ring of three wraps
loop1[2432-K64]           2432 x 2304            <A_F32, 2, 6>                 t0 = 152 < 160                 just outside the rule: small tile, MT = 38, NT = 12
loop1[4224-K64]           4224 x 2304            <A_F32, 2, 6>                 256 < t0 = 264 < 512           just outside: small tile, MT = 66
loop1[2560-K32]           2560 x 2304            <A_F32, 2, 6>                 K = 32 < 64 (T = 1)            the rule that protects the ring's tail; MT = 40: XCD map
big[8192-*]               8192 x 2304 (768 x 3)  <fp16|pairs|int8, 4, 9>,      t0 = 512, waste 1.0            two per CU; MT = 64: XCD map; T = 1; S = 512
                                                 <A_F32, 4, 9, 2>
big[8208-*]               8208 x 2304            the same four                 t0 = 520, waste 1.014          65 row tiles, the last ragged; linear map; T = 2; S = 48 transposed (div_magic)
big[4736-*]               4736 x 3840 (1280 x 3) the same four                 t0 = 37 * 14 = 518, waste 1.05 ragged last column tile (96 of 288 columns), boundaries at column 128 (wave wn = 0's
                                                                                                              half) and 256 (wn = 1's half) of a tile; T = 3; linear map
                          (E = 736 is not a multiple of 64 and the ABI refuses it: E = 1280 is the smallest three-segment width with a ragged last 288 tile inside waste <= 1.06)
saturation[*]             80 x 192               <fp16|fp32|int8, 2, 6>        t0 = 1                         the fma itself +-inf (alpha = 2^126), a finite value whose quotient overflows (2^100 / 2^-40):
                                                                                                              values and no-values bodies, 16-bit and int8 epilogue forms
random[*]                 one per kernel (9)     all nine                      as above                       random data against float64 products: the bar of test_proj_gpu.py
int8 cases run through `_lib.load().oeh_proj_quant_i8` with acc_add (ops.proj_quant_i8 takes no int8); a case with a values-only
segment or y_stride_row > E too; all others through ops.proj_quant_i8(_outs=...)."""
import ctypes as C
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

FORM_CODE = {"fp16": 0, "pairs": 1, "fp32": 2, "int8": 3}
VR, VT, V, R, T = "values+row", "values+transposed", "values", "row", "transposed"
SENT_I8, SENT_F32 = 0x5B, -7777.25
DEV = "cuda"
ZP_IN = 117   # the int8 form's acc_add = (128 - ZP_IN) * column sums of w: the producer's zero point


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from outeffhop_amd import ops as _ops

    return _ops


def host_rule(form, M, N, K):
    """launch_gemm's choice (csrc/oeh_gemm.hip): (MI, NJ, LOOP, tile map)."""
    t0 = ((M + 127) // 128) * ((N + 287) // 288)
    waste = t0 * 128.0 * 288.0 / (float(M) * float(N))
    if t0 >= 512 and waste <= 1.06:
        mi, nj, loop = 4, 9, (2 if form == "fp32" else 0)
    elif form == "fp32" and 160 <= t0 <= 256 and waste <= 1.06 and K >= 64:
        mi, nj, loop = 4, 9, 1
    else:
        mi, nj, loop = 2, 6, 0
    mt = (M + 32 * mi - 1) // (32 * mi)
    return mi, nj, loop, ("xcd" if mt % 8 == 0 else "linear")


def _guarded(n_elem, dtype, margin):
    """A flat buffer of sentinels with `margin` elements on either side of the n_elem the kernel may write."""
    buf = torch.full((n_elem + 2 * margin,), SENT_I8 if dtype == torch.int8 else SENT_F32, dtype=dtype, device="cuda")
    return buf, buf[margin:margin + n_elem]


def _margins_intact(buf, n_elem, margin):
    s = SENT_I8 if buf.dtype == torch.int8 else SENT_F32
    return bool((buf[:margin] == s).all()) and bool((buf[margin + n_elem:] == s).all())


def _padded(t, pad, fill):
    """t (rows, cols) as the first columns of a (rows, cols + pad) buffer whose pad columns hold `fill`."""
    if pad == 0:
        return t.contiguous()
    buf = torch.full((t.shape[0], t.shape[1] + pad), fill, dtype=t.dtype, device=t.device)
    buf[:, :t.shape[1]] = t
    return buf[:, :t.shape[1]]


def _operands(ops, form, M, N, K, seed):
    """(a64, w64, unit, a, w): the exact values as float64 and the tensors the kernel reads.  fp16: multiples of 2^-4 below 31 (10 bits);
    pairs / fp32: integers up to 31 + multiples of 2^-9 (14 bits: the lo half is needed); weights in [-8, 8); int8: both full range."""
    g = torch.Generator().manual_seed(seed)
    if form == "int8":
        a64 = torch.randint(-128, 128, (M, K), generator=g).double().to(DEV)
        w64 = torch.randint(-128, 128, (N, K), generator=g).double().to(DEV)
        return a64, w64, 1.0, a64.to(torch.int8), w64.to(torch.int8)
    w64 = torch.randint(-8, 8, (N, K), generator=g).double().to(DEV)
    w = w64.to(torch.float16)
    if form == "fp16":
        unit = 2.0 ** -4
        a64 = torch.randint(-31 * 16, 31 * 16 + 1, (M, K), generator=g).double().to(DEV) * unit
        a = a64.to(torch.float16)
        assert torch.equal(a.double(), a64)
        return a64, w64, unit, a, w
    unit = 2.0 ** -9
    a64 = torch.randint(-31 * 512 - 511, 31 * 512 + 512, (M, K), generator=g).double().to(DEV) * unit
    a32 = a64.float()
    assert torch.equal(a32.double(), a64)
    assert bool((a32.half().float() != a32).any())          # more than fp16's 11 bits: hi alone is not x
    if form == "fp32":
        return a64, w64, unit, a32, w
    p = ops.split_pairs(a32)                                 # [hi | lo 2^11]
    assert bool((p[:, K:] != 0).any())                       # the lo half is needed ...
    assert torch.equal(p[:, :K].double() + p[:, K:].double() * 2.0 ** -11, a64)   # ... and the pair is x exactly
    return a64, w64, unit, p, w


def _problem(ops, form, B, S, E, K, forms, zps, seed, sat=False):
    """Operands, per-segment (alpha, scale, zp), bias, acc_add and the exact expected indices / values."""
    n, M = len(forms), B * S
    N = n * E
    a64, w64, unit, a, w = _operands(ops, form, M, N, K, seed)
    acc = a64 @ w64.t()                                        # exact: integers * unit far below 2^53
    bound = float((a64.abs() @ w64.abs().t()).max()) / unit    # any partial sum in any order (pairs: + |lo| |w| <= 2^-6 of it)
    add = None
    if form == "int8":
        add = ((128 - ZP_IN) * w64.sum(dim=1)).to(torch.int32).contiguous()
        acc = acc + add.double()[None, :]
        bound += float(add.abs().max())
    assert bound * (1.0 + 2.0 ** -6) < 2.0 ** 24, bound
    sigma = float(acc.std()) / unit
    s_exp = max(1, int(math.floor(math.log2(sigma / 128.0))))  # step = 2^s_exp grid units: quotients with a standard deviation of 128-256 steps
    g = torch.Generator().manual_seed(seed + 1)
    segs, bias64, exp = [], torch.zeros(N, dtype=torch.float64, device=DEV), []
    rows = torch.arange(E, device=DEV)
    for i in range(n):
        alpha = 2.0 ** (-6 - i)
        grid = alpha * unit
        zp = float(zps[i % len(zps)])
        acc_i = acc[:, i * E:(i + 1) * E] / unit                # integers
        if sat and i < 2:
            # i = 0: the fma alpha * acc + bias is +-inf for |acc| >= 4; i = 1: finite values (<= 2^124) whose quotient by 2^-40 overflows
            alpha, scale = (2.0 ** 126, 2.0 ** 100) if i == 0 else (2.0 ** 100, 2.0 ** -40)
            grid = alpha * unit
            b_g = torch.randint(-3, 4, (E,), generator=g).double().to(DEV)
        else:
            scale = grid * 2.0 ** s_exp
            # the bias puts row (7 c + 3) % M of column c exactly on the tie k + 0.5 with index k + zp in [2, 251]; otherwise it is random
            k = 2.0 + ((37 * rows) % 250).double() - zp
            b_g = (k + 0.5) * 2.0 ** s_exp - acc_i[(7 * rows + 3) % M, rows]
        bias64[i * E:(i + 1) * E] = b_g * grid
        v_g = acc_i + b_g[None, :]
        assert float(v_g.abs().max()) < 2.0 ** 24               # alpha * acc + bias is exact in fp32 (where it is finite)
        v = v_g * grid
        q = v / scale
        idx = torch.clamp(torch.round(q) + zp, 0, 255)
        if not sat:
            tie = ((q - torch.floor(q)) == 0.5) & (q + zp > 0) & (q + zp < 255)
            assert bool((idx == 0).any()) and bool((idx == 255).any()) and int(tie.sum()) >= 1
        elif i < 2:
            assert bool((idx == 0).any()) and bool((idx == 255).any())
            assert float(v.abs().max()) > 3.5e38 if i == 0 else (float(v.abs().max()) < 3.4e38 and float(v.abs().max()) / scale > 3.5e38)
        exp.append((idx.to(torch.int16), (scale * (idx - zp)).float()))
        segs.append((alpha, scale, zp))
    bias = bias64.float()
    assert torch.equal(bias.double(), bias64)
    return a, w, bias, add, segs, exp


def _launch(ops, form, a, w, bias, add, B, S, E, K, segs, forms, y_pad=0, via=None):
    """One call; returns per segment (index tensor (M, E) int16 in row order or None, values (M, E) or None) read back from guarded buffers,
    after the margins and pads have been checked."""
    from outeffhop_amd import _lib

    n, M, H = len(forms), B * S, E // 64
    margin = 16 * max(256, 12 * E)
    bufs, outs = [], []
    for f in forms:
        ob = yb = None
        if f in (VR, VT, R, T):
            ob = _guarded(M * E, torch.int8, margin)
        if f in (VR, VT, V):
            yb = _guarded(M * (E + y_pad), torch.float32, margin)
        bufs.append((ob, yb))
    abi = via == "abi" or form == "int8" or y_pad != 0 or any(f == V for f in forms)
    if abi:
        arr = (_lib.oeh_proj_seg * n)()
        for i, f in enumerate(forms):
            ob, yb = bufs[i]
            arr[i].alpha, arr[i].scale, arr[i].zero_point = segs[i]
            arr[i].out = ob[1].data_ptr() if ob else None
            arr[i].y = yb[1].data_ptr() if yb else None
            arr[i].y_stride_row, arr[i].transpose = E + y_pad, int(f in (VT, T))
            arr[i].acc_add = add[i * E:(i + 1) * E].data_ptr() if add is not None else None
        rc = _lib.load().oeh_proj_quant_i8(a.data_ptr(), FORM_CODE[form], w.data_ptr(), bias.data_ptr(), B, S, K, E, n, arr, a.stride(0), w.stride(0),
                                           C.c_void_p(torch.cuda.current_stream().cuda_stream))
        _lib.check(rc, "oeh_proj_quant_i8")
    else:
        o = [(ob[1].view((B, H, 64, S) if f in (VT, T) else (B, S, E)), yb[1].view(B, S, E) if yb else None) for f, (ob, yb) in zip(forms, bufs)]
        ops.proj_quant_i8(a, w, bias, B, S, [(al, ops.FakeQuantSpec(sc, zp), f in (VT, T), f in (VR, VT)) for (al, sc, zp), f in zip(segs, forms)],
                          pairs=(form == "pairs"), _outs=o)
    torch.cuda.synchronize()
    for i, f in enumerate(forms):
        ob, yb = bufs[i]
        idx = y = None
        if ob:
            assert _margins_intact(ob[0], M * E, margin), (i, f, "index margins")
            idx = ob[1].view(B, H, 64, S).permute(0, 3, 1, 2).reshape(M, E) if f in (VT, T) else ob[1].view(M, E)
            idx = idx.to(torch.int16) + 128
        if yb:
            assert _margins_intact(yb[0], M * (E + y_pad), margin), (i, f, "value margins")
            y2 = yb[1].view(M, E + y_pad)
            assert bool((y2[:, E:] == SENT_F32).all()), (i, f, "value pad columns")
            y = y2[:, :E]
        outs.append((idx, y))
    return outs


def _check(outs, exp, forms, what):
    for i, f in enumerate(forms):
        idx, y = outs[i]
        e_idx, e_y = exp[i]
        if idx is not None:
            assert torch.equal(idx, e_idx), (what, i, f, "indices", int((idx != e_idx).sum()), torch.nonzero(idx != e_idx)[:4].tolist())
        if y is not None:
            assert torch.equal(y, e_y), (what, i, f, "values", int((y != e_y).sum()), torch.nonzero(y != e_y)[:4].tolist())
            # the sign of zero: the reference's scale * (idx - zp) is never -0
            assert torch.equal(y.contiguous().view(torch.int32), e_y.contiguous().view(torch.int32)), (what, i, f, "value bits (-0.0)")


def _k(form, K):
    return 2 * K if form == "int8" else K   # the same number of K steps: a step is 64 bytes of a row


def _exact_case(ops, form, B, S, E, K, forms, zps, kernel, seed, lda_pad=0, ldw_pad=0, y_pad=0):
    K = _k(form, K)
    M, N = B * S, len(forms) * E
    assert host_rule(form, M, N, K) == kernel, host_rule(form, M, N, K)
    a, w, bias, add, segs, exp = _problem(ops, form, B, S, E, K, forms, zps, seed)
    eb = {"fp16": 2, "pairs": 2, "fp32": 4, "int8": 1}[form]
    a = _padded(a, lda_pad * (16 // eb), 127 if form == "int8" else float("nan"))
    w = _padded(w, ldw_pad * (16 if form == "int8" else 8), 127 if form == "int8" else float("nan"))
    outs = _launch(ops, form, a, w, bias, add, B, S, E, K, segs, forms, y_pad=y_pad)
    _check(outs, exp, forms, (form, M, N, K))
    return outs


FORMS4 = ["fp16", "pairs", "fp32", "int8"]
SMALL = {   # B, S, E, K, forms, zero points, tile map, lda_pad, ldw_pad (16-byte pieces), y_pad
    "tail": (1, 16, 64, 32, [VR], [117], "linear", 0, 0, 0),
    "ragged": (5, 16, 64, 64, [VT, R, VR], [0, 255, 117], "linear", 1, 3, 0),
    "xcd": (32, 16, 128, 96, [R, VT, V], [255, 117, 0], "xcd", 0, 0, 0),
    "linear": (12, 48, 64, 64, [T, VR], [117, 0], "linear", 2, 1, 32),
}


@pytest.mark.parametrize("form", FORMS4)
@pytest.mark.parametrize("case", list(SMALL))
def test_small_tile_exact(ops, case, form):
    """<form, 2, 6>: one mostly-tail tile; ragged rows; both tile maps; segment boundaries inside a tile; T = 1, 2, 3; lda, ldw, y_stride_row beyond the
    row; a transposed segment whose row tile spans batch elements (S = 16, 48)."""
    B, S, E, K, forms, zps, tmap, lda_pad, ldw_pad, y_pad = SMALL[case]
    _exact_case(ops, form, B, S, E, K, forms, zps, (2, 6, 0, tmap), 100 + len(case), lda_pad, ldw_pad, y_pad)


@pytest.mark.parametrize("form", FORMS4)
@pytest.mark.parametrize("rot", range(5))
def test_every_epilogue_form_in_every_segment_position(ops, rot, form):
    """The five per-segment forms in positions 0, 1, 2 (rotation `rot` puts form (rot + p) % 5 in position p), zero points 0, 255, 117 rotating
    with them; M = 240 = 5 x 48 (ragged against the 64-row tile, a transposed row tile spans two batch elements)."""
    five = [VR, VT, V, R, T]
    forms = [five[(rot + p) % 5] for p in range(3)]
    zps = [[0.0, 255.0, 117.0][(rot + p) % 3] for p in range(3)]
    _exact_case(ops, form, 5, 48, 64, 32, forms, zps, (2, 6, 0, "linear"), 200 + rot)


@pytest.mark.parametrize("form", FORMS4)
def test_values_on_and_off_give_the_same_indices(ops, form):
    """The same problem with values (the clamp is v_med3_f32) and without (the clamp is v_cvt_pk_u8_f32's saturation), zero points 0, 255, 117."""
    on = _exact_case(ops, form, 5, 16, 64, 64, [VR, VT, VR], [0, 255, 117], (2, 6, 0, "linear"), 300)
    off = _exact_case(ops, form, 5, 16, 64, 64, [R, T, R], [0, 255, 117], (2, 6, 0, "linear"), 300)
    for (i_on, _), (i_off, _) in zip(on, off):
        assert torch.equal(i_on, i_off)


LOOP1 = {   # B, S, K, forms, expected kernel
    "2560-K64": (160, 16, 64, [R, T, VR], (4, 9, 1, "linear")),
    "2576-K96": (161, 16, 96, [VT, R, R], (4, 9, 1, "linear")),
    "4096-K128": (256, 16, 128, [R, VR, T], (4, 9, 1, "xcd")),
    "2432-K64": (152, 16, 64, [R, T, VR], (2, 6, 0, "linear")),
    "4224-K64": (88, 48, 64, [T, R, VR], (2, 6, 0, "linear")),
    "2560-K32": (160, 16, 32, [VR, T, R], (2, 6, 0, "xcd")),
}


@pytest.mark.parametrize("case", list(LOOP1))
def test_one_workgroup_per_cu_loop_and_its_borders_exact(ops, case):
    """<A_F32, 4, 9, LOOP = 1> (160 <= tiles <= 256, K >= 64): T = 2 (the two-step tail alone), 3, 4 (the ring of three wraps), both tile maps, a
    ragged last row tile - and the shapes just outside the rule, which must take the small tile (T = 1 would break the tail)."""
    B, S, K, forms, kernel = LOOP1[case]
    _exact_case(ops, "fp32", B, S, 768, K, forms, [117, 0, 255], kernel, 400 + K)


BIG = {   # B, S, E, K, forms, tile map
    "8192": (16, 512, 768, 32, [V, T, R], "xcd"),
    "8208": (171, 48, 768, 64, [VR, R, T], "linear"),
    "4736": (296, 16, 1280, 96, [T, VT, R], "linear"),
}


@pytest.mark.parametrize("form", FORMS4)
@pytest.mark.parametrize("case", list(BIG))
def test_large_tile_exact(ops, case, form):
    """<form, 4, 9> (fp32: LOOP = 2), two workgroups per CU: exact rows and columns; a ragged last row tile on the linear map; a ragged last column
    tile with segment boundaries inside both waves' halves of a tile; T = 1, 2, 3."""
    B, S, E, K, forms, tmap = BIG[case]
    _exact_case(ops, form, B, S, E, K, forms, [0, 117, 255], (4, 9, 2 if form == "fp32" else 0, tmap), 500 + E)


@pytest.mark.parametrize("values", [True, False], ids=["values", "indices-only"])
@pytest.mark.parametrize("form", ["fp16", "fp32", "int8"])
def test_epilogue_saturates_where_the_value_or_its_quotient_overflows(ops, form, values):
    """Segment 0: alpha = 2^126 / unit - the fma alpha * acc + bias itself is +-inf; segment 1: values up to 2^124 against a step of 2^-40 - finite,
    the product with 1 / step overflows; segment 2: an ordinary grid.  The reference's clamp(round(v / scale) + zp, 0, 255) gives 255 and
    scale * (255 - zp) for positive, 0 and scale * (0 - zp) for negative inputs (fq_quot's residual turned both into NaN -> index 0)."""
    forms = [VR, VT, V] if values else [R, T, R]
    B, S, E, K = 5, 16, 64, _k(form, 64)
    assert host_rule(form, B * S, 3 * E, K) == (2, 6, 0, "linear")
    a, w, bias, add, segs, exp = _problem(ops, form, B, S, E, K, forms, [117, 0, 255], 600, sat=True)
    outs = _launch(ops, form, a, w, bias, add, B, S, E, K, segs, forms)
    _check(outs, exp, forms, (form, "saturation"))


def _grid(v64):
    lo, hi = v64.min().item() * 0.9, v64.max().item() * 0.9  # (a little clipping at both ends)
    sc = np.float32((hi - lo) / 255.0)
    return float(sc), float(np.clip(np.rint(-lo / sc), 0, 255))


RANDOM = {   # form, B, S, E, K -> kernel
    "fp16-2x6": ("fp16", 25, 16, 64, 96, (2, 6, 0)), "pairs-2x6": ("pairs", 25, 16, 64, 96, (2, 6, 0)),
    "fp32-2x6": ("fp32", 25, 16, 64, 96, (2, 6, 0)), "int8-2x6": ("int8", 25, 16, 64, 128, (2, 6, 0)),
    "fp32-4x9-loop1": ("fp32", 160, 16, 768, 96, (4, 9, 1)),
    "fp16-4x9": ("fp16", 16, 512, 768, 96, (4, 9, 0)), "pairs-4x9": ("pairs", 16, 512, 768, 96, (4, 9, 0)),
    "fp32-4x9-loop2": ("fp32", 16, 512, 768, 96, (4, 9, 2)), "int8-4x9": ("int8", 16, 512, 768, 128, (4, 9, 0)),
}


@pytest.mark.parametrize("case", list(RANDOM))
def test_random_data_per_kernel_against_float64(ops, case):
    """One random-data case per kernel against float64 products, the bar of test_proj_gpu.py: every index within one step of the exact one, the
    rate of differing indices at most max(3e-5, 3 x the rate of the library GEMM + quantize_heads_i8 path on the same operands)."""
    form, B, S, E, K, kernel = RANDOM[case]
    M, N, H = B * S, 3 * E, E // 64
    assert host_rule(form, M, N, K)[:3] == kernel
    torch.manual_seed(sum(map(ord, case)))
    if form == "int8":
        a = torch.randint(-128, 128, (M, K), device="cuda").to(torch.int8)
        w = torch.randint(-128, 128, (N, K), device="cuda").to(torch.int8)
        a64, alphas = a.double(), [3.1e-5, 2.5e-5, 2.0e-5]
        a_lib, w_lib = a.to(torch.float16), w.to(torch.float16).t().contiguous()   # exact products, fp32 sums of integers below 2^24
    else:
        x = torch.randn(M, K, device="cuda")
        x[:, ::37] *= 30.0
        w = torch.randint(-128, 128, (N, K), device="cuda").to(torch.float16)
        alphas = [0.003, 0.0025, 0.002]
        if form == "fp16":
            a = x.to(torch.float16)
            a64, a_lib, w_lib = a.double(), a, w.t().contiguous()
        else:
            a_lib = ops.split_pairs(x)
            a = a_lib if form == "pairs" else x
            a64, w_lib = x.double(), torch.cat([w, w * 2.0 ** -11], dim=1).t().contiguous()
    bias = torch.randn(N, device="cuda") * 0.1
    ref64 = a64 @ w.double().t()
    acc_lib = torch.mm(a_lib, w_lib, out_dtype=torch.float32).view(B, S, N)
    vals = [ref64[:, n * E:(n + 1) * E] * alphas[n] + bias[n * E:(n + 1) * E].double() for n in range(3)]
    grids = [_grid(v) for v in vals]
    forms = [R, VR, T]
    segs = [(alphas[n], grids[n][0], grids[n][1]) for n in range(3)]
    outs = _launch(ops, form, a, w, bias, None, B, S, E, K, segs, forms)
    for n in range(3):
        sc, zp = np.float32(grids[n][0]), grids[n][1]
        ex = torch.clamp(torch.round(vals[n] / float(sc)) + zp, 0, 255).to(torch.int16)
        old = ops.quantize_heads_i8(acc_lib[..., n * E:(n + 1) * E], ops.FakeQuantSpec(float(sc), zp), H, alpha=alphas[n], bias=bias[n * E:(n + 1) * E].contiguous())
        old = old.permute(0, 2, 1, 3).reshape(M, E).to(torch.int16) + 128
        d, d_old = (outs[n][0] - ex).abs(), (old - ex).abs()
        rate, rate_old = float((d != 0).float().mean()), float((d_old != 0).float().mean())
        print(f"{case} [{'qkv'[n]}]: index != exact {rate:.1e} (library GEMM + quantiser pass: {rate_old:.1e}), max {int(d.max())} step")
        assert int(d.max()) <= 1 and rate <= max(3e-5, 3.0 * rate_old)
        if outs[n][1] is not None:
            assert torch.equal(outs[n][1], sc * (outs[n][0].float() - np.float32(zp)))
