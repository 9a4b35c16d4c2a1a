"""The one-pass kernel's two launch forms (csrc/oeh_attn_params.h: AttnHot).  The plain 16-bit forms take what the block-id decode and the
Q / K / V requests read as 14 leading scalar kernel arguments, which gfx950 preloads into SGPRs; include/oeh_debug.h bit 13 forces the
launch from the AttnParams block alone.  Both forms run the same kernel body on the same values, so the outputs must be the same bits;
the prefix form also meets the oracle under the tolerances of tests/test_attn_gpu.py for the dtype.

Shapes: the smallest at which the decode or the addresses can go wrong -
  B=3 H=5 S=130 causal     B*H = 15 is padded to 16 block columns (early-return blocks), ragged last q tile
  B=2 H=12 S=512 causal    the headline body: with two query blocks per wave (forced) the four q-tile classes of S=512
  (B,S,H,d) permuted views and (B,H,S,d) contiguous tensors: both sets of strides
  Sq=64 Sk=192 causal      the diagonal offset by Sk - Sq (q is the last 64 rows of a 192-row storage: with storages of their own, q's batch
                           stride differs from k's and the launch is not the prefix form)
  q / k / v with different strides: not the prefix form (one set of strides in the prefix) - the launch counter must not move
  bf16                     the second 16-bit instantiation
each with one and with two query blocks per wave."""
import numpy as np
import pytest

from oracle import oeh_oracle as O

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

NO_HOT = 1 << 13       # include/oeh_debug.h: the AttnParams-only launch form
FORCE_FLASH = 1 << 8   # the one-pass kernel also where the library would pick the full-row kernel (short rows)
BF16_TOL = dict(atol=2e-2, rtol=2e-2)   # tests/test_attn_gpu.py


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from outeffhop_amd import ops as _ops

    return _ops


@pytest.fixture(scope="module")
def lib():
    import ctypes as C

    from outeffhop_amd import _lib

    lb = _lib.load()
    lb.oeh_debug_hot_launches.restype = C.c_long
    return lb


def _np32(t):
    return t.detach().float().cpu().numpy()


def _check(got, want, dtype, msg):
    """tests/test_attn_gpu.py: fp16 - 1e-3 + half an fp16 ulp of the reference; bf16 - atol = rtol = 2e-2"""
    got = _np32(got)
    err = np.abs(got - want)
    if dtype == torch.float16:
        lim = np.float32(1e-3) + 0.5 * np.spacing(np.abs(want).astype(np.float16)).astype(np.float32)
    else:
        lim = BF16_TOL["atol"] + BF16_TOL["rtol"] * np.abs(want)
    assert np.isfinite(got).all(), f"{msg}: non-finite output"
    assert float((err - lim).max()) <= 0, f"{msg}: max abs err {err.max():.3e} at {np.unravel_index((err - lim).argmax(), err.shape)}"


def _inputs(B, H, Sq, Sk, D, dtype, layout, seed):
    """logical (B,H,S,D) tensors.  layout "bshd": permuted views of (B,S,H,D) storage (how the models call); "bhsd": contiguous;
    "mixed": q as a permuted view, k contiguous, v a permuted view of a wider row (three different sets of strides);
    "qslice": "bshd" with q the last Sq rows of an Sk-row storage (q shares k's and v's strides although Sq != Sk)."""
    g = torch.Generator().manual_seed(seed)

    def one(S, lay, scale=1.0):
        x = (torch.randn((B, H, S, D), generator=g) * scale).to(dtype).cuda()
        if lay == "bhsd":
            return x
        if lay == "qslice":
            st = torch.zeros((B, Sk, H, D), dtype=dtype, device="cuda")
            st[:, Sk - S:] = x.permute(0, 2, 1, 3)
            return st[:, Sk - S:].permute(0, 2, 1, 3)
        if lay == "wide":  # rows of 2 D elements, the first D used
            st = torch.zeros((B, S, H, 2 * D), dtype=dtype, device="cuda")
            st[..., :D] = x.permute(0, 2, 1, 3)
            return st[..., :D].permute(0, 2, 1, 3)
        return x.permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3)

    lays = {"bshd": ("bshd",) * 3, "bhsd": ("bhsd",) * 3, "mixed": ("bshd", "bhsd", "wide"), "qslice": ("qslice", "bshd", "bshd")}[layout]
    return one(Sq, lays[0], D ** -0.5), one(Sk, lays[1]), one(Sk, lays[2])


CASES = [
    # name,            B, H,  Sq,  Sk,  D, dtype,           layout,  prefix form expected
    ("pad16_ragged",   3, 5,  130, 130, 64, torch.float16,  "bshd",  True),
    ("headline_body",  2, 12, 512, 512, 64, torch.float16,  "bshd",  True),
    ("contiguous",     2, 3,  192, 192, 64, torch.float16,  "bhsd",  True),
    ("offset_diag",    2, 3,  64,  192, 64, torch.float16,  "qslice", True),
    ("mixed_strides",  2, 3,  192, 192, 64, torch.float16,  "mixed", False),
    ("bf16",           3, 5,  130, 130, 64, torch.bfloat16, "bshd",  True),
]


@pytest.fixture(scope="module")
def references():
    """name -> (q, k, v, oracle output), computed once for both values of mq"""
    out = {}
    for n, (name, B, H, Sq, Sk, D, dtype, layout, _) in enumerate(CASES):
        q, k, v = _inputs(B, H, Sq, Sk, D, dtype, layout, 9100 + n)
        out[name] = (q, k, v, O.attn_core(_np32(q), _np32(k), _np32(v), causal=True, clamp_min=True))
    return out


@pytest.mark.parametrize("mq", [1, 2])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_prefix_form_equals_struct_form_and_meets_the_oracle(ops, lib, references, case, mq):
    name, B, H, Sq, Sk, D, dtype, layout, expect_hot = case
    q, k, v, want = references[name]
    kw = dict(causal=True, clamp_min=True)
    try:
        assert lib.oeh_debug_set_variant(FORCE_FLASH, mq) == 0
        n0 = lib.oeh_debug_hot_launches()
        a = ops.attn_fwd(q, k, v, **kw)
        n1 = lib.oeh_debug_hot_launches()
        assert lib.oeh_debug_set_variant(FORCE_FLASH | NO_HOT, mq) == 0
        b = ops.attn_fwd(q, k, v, **kw)
        n2 = lib.oeh_debug_hot_launches()
    finally:
        lib.oeh_debug_set_variant(0, 0)
    assert n1 - n0 == (1 if expect_hot else 0), f"{name} mq={mq}: launch form (prefix launches {n1 - n0})"
    assert n2 == n1, f"{name} mq={mq}: the hook did not force the AttnParams-only form"
    assert torch.equal(a, b), f"{name} mq={mq}: the two launch forms differ"
    _check(a, want, dtype, f"{name} mq={mq}")


def test_library_default_takes_the_prefix_form_on_the_headline_geometry(ops, lib, references):
    """no hook set: what production launches (B*H and S of the headline's kind, smaller batch)"""
    q, k, v, want = references["headline_body"]
    assert ops.attn_variant(2, 12, 512, 512, 64, torch.float16, causal=True).startswith("flash16/")
    n0 = lib.oeh_debug_hot_launches()
    a = ops.attn_fwd(q, k, v, causal=True, clamp_min=True)
    assert lib.oeh_debug_hot_launches() - n0 == 1
    _check(a, want, torch.float16, "library default")
