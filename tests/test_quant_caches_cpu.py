"""The host-side caches of the quantised path (no GPU): the tensor watch they all key on, QuantLinear's weight-derived forms - exact
values, no rebuild without a change, a rebuild after every kind of change - and the frozen-8-bit predicate the INT8 route composes."""
import numpy as np
import pytest
import torch

from outeffhop_amd import quantization as Q


def test_watch_sees_every_kind_of_change_on_bare_dicts():
    from outeffhop_amd._watch import TensorWatch, cached

    a, b = {"w": torch.zeros(4), "none": None}, {"r": torch.ones(2)}
    slots = [(a, "w"), (a, "none"), (b, "r"), (b, "missing")]
    assert TensorWatch(slots).unchanged()
    w = TensorWatch(slots)
    a["w"].sum(), b["r"].clone(), a["w"].view(2, 2)                         # reads and views are no change
    assert w.unchanged() and w.unchanged()
    assert [t is u for t, u in zip(w.tensors(), (a["w"], b["r"]))] == [True, True]  # (the held tensors, None left out)
    a["w"].add_(1.0)                                                          # an in-place write: the version counter
    assert not w.unchanged()
    w = TensorWatch(slots)
    a["w"].data = torch.full((4,), 7.0)                                       # `.data = other`: same object, same version - the address
    assert not w.unchanged()
    w = TensorWatch(slots)
    b["r"] = b["r"].clone()                                                   # the slot rebound to another (equal) tensor
    assert not w.unchanged()
    w = TensorWatch(slots)
    a["none"] = torch.zeros(1)                                                # None -> tensor
    assert not w.unchanged()
    w = TensorWatch(slots)
    a["none"] = None                                                          # tensor -> None
    assert not w.unchanged()
    w = TensorWatch(slots)
    b["missing"] = torch.zeros(1)                                             # a name that was absent counts as None
    assert not w.unchanged()
    # a 0-dim tensor replaced again and again (the allocator hands the freed address out again): the watch holds the old object, so the
    # new one cannot sit at its address
    w = TensorWatch([(b, "r")])
    for flip in range(8):
        b["r"] = torch.tensor(bool(flip & 1))
        assert not w.unchanged()
        w = TensorWatch([(b, "r")])
        assert w.unchanged()
    # `cached`: built once, again when the plain key or a watched slot changes
    store, built = {}, []
    get = lambda key: cached(store, "c", key, lambda: [(a, "w")], lambda: built.append(key) or len(built))  # noqa: E731
    assert (get(1), get(1), get(2), get(2)) == (1, 1, 2, 2)
    a["w"].mul_(2.0)
    assert (get(2), get(2)) == (3, 3) and built == [1, 2, 2]


def _lin(act_method=Q.AsymmetricUniformQuantizer, n_bits_act=8, seed=5):
    """A CPU QuantLinear 64 -> 128: symmetric 8-bit weights, weight range estimated (min-max) then fixed; output range set."""
    torch.manual_seed(seed)
    m = Q.QuantLinear(64, 128, method=Q.SymmetricUniformQuantizer, act_method=act_method, n_bits=8, n_bits_act=n_bits_act).eval()
    m.quantized_weights()
    with torch.no_grad():
        m.weight_quantizer(m.weight)
    m.weight_quantizer.fix_ranges()
    m.activation_quantizer.set_quant_range(-1.5, 2.5)
    return m


def _expect(m):
    """(Iw fp32 (N, K), float32-rounded scale) from the definition: clamp(round(w / scale)) on the weight quantiser's grid."""
    qz = m.weight_quantizer.quantizer
    scale = torch.clamp(qz._delta, min=qz.eps)
    signed = bool(qz._signed)
    lo, hi = (-(2.0 ** (qz.n_bits - 1)), 2.0 ** (qz.n_bits - 1) - 1) if signed else (0.0, 2.0 ** qz.n_bits - 1)
    return torch.clamp(torch.round(m.weight.detach() / scale), lo, hi), float(np.float32(float(scale)))


def _check_forms(m):
    iw, s32 = _expect(m)
    ww, s_pair = m._pair_weights()
    assert ww.dtype == torch.float16 and ww.shape == (128, 128) and ww.is_contiguous()
    assert torch.equal(ww, torch.cat([iw.t(), iw.t() / 2048.0], dim=0).to(torch.float16))
    wi, s_int = m._int_weights()
    assert wi.dtype == torch.float16 and torch.equal(wi, iw.to(torch.float16)) and wi.is_contiguous()
    i8, add, s_i8 = m._int8_weights(3.0)
    assert i8.dtype == torch.int8 and torch.equal(i8, iw.to(torch.int8)) and torch.equal(i8.float(), iw)
    assert add.dtype == torch.int32 and torch.equal(add, ((128 - 3) * iw.to(torch.int64).sum(dim=1)).to(torch.int32))
    assert s_pair == s_int == s_i8 == s32 and isinstance(s_pair, float)
    assert m._int8_weights_fit() is True
    return ww, wi, i8, add


def test_quantlinear_weight_forms_are_exact_and_rebuilt_only_after_a_change():
    m = _lin()
    assert float(m.weight.detach().min()) < 0 < float(m.weight.detach().max()) and m.weight_quantizer.quantizer.signed
    first = _check_forms(m)
    again = (m._pair_weights()[0], m._int_weights()[0], *m._int8_weights(3.0)[:2])
    assert all(a is b for a, b in zip(first, again)), "a form was rebuilt although nothing changed"
    assert not torch.equal(m._int8_weights(5.0)[1], first[3]) and torch.equal(m._int8_weights(3.0)[1], first[3])  # (xzero is part of the key)

    def change_mul(m):
        with torch.no_grad():
            m.weight.mul_(0.75)

    def change_data(m):
        m.weight.data = m.weight.data * 0.5 + 0.001

    def change_range(m):
        m.weight_quantizer.set_quant_range(2.0 * float(m.weight.detach().min()), 2.0 * float(m.weight.detach().max()))

    def change_bits(m):
        m.weight_quantizer.quantizer.n_bits = 4

    for change in (change_mul, change_data, change_range, change_bits):
        m = _lin()
        before = _check_forms(m)
        old = [t.clone() for t in before]
        change(m)
        after = _check_forms(m)                                                # exact on the new state ...
        assert all(a is not b for a, b in zip(before, after)), change.__name__
        assert not torch.equal(after[1], old[1]), change.__name__              # ... which is another matrix
        assert all(a is b for a, b in zip(after, _check_forms(m))), change.__name__


def test_unsigned_weight_grid_is_never_served_from_a_stale_int8_answer():
    """set_quant_range assigns fresh 0-dim buffers each time: version 0, and the allocator reuses their addresses.  A key of
    (data_ptr, _version) pairs can therefore repeat across a signed -> unsigned flip of the weight grid (integers up to 255: they would
    wrap as int8); a watch that holds the buffer objects cannot."""
    m = _lin()
    m.quantized_acts()
    m.activation_quantizer.fix_ranges()
    wmin, wmax = float(m.weight.detach().min()), float(m.weight.detach().max())
    assert m.out_fixed8 and m.int8_index_ok(32)
    for _ in range(6):
        m.weight_quantizer.set_quant_range(0.0, wmax)                          # unsigned: [0, 255]
        iw, _ = _expect(m)
        assert float(iw.max()) == 255.0 and not m.weight_quantizer.quantizer.signed
        assert m._int8_weights_fit() is False and m.int8_index_ok(32) is False
        with pytest.raises(ValueError, match="do not fit int8"):
            m._int8_weights(3.0)
        assert torch.equal(m._int_weights()[0], iw.to(torch.float16))          # (the fp16-integer form serves them)
        m.weight_quantizer.set_quant_range(wmin, wmax)                         # signed again
        assert m._int8_weights_fit() is True and m.int8_index_ok(32) is True
        _check_forms(m)


def test_frozen_8bit_output_quantiser_predicate():
    m = _lin()
    assert not m.out_fixed8                                                    # acts off
    m.quantized_acts()
    assert m.activation_quantizer.state == Q.Qstates.estimate_ranges and not m.out_fixed8  # estimating
    m.activation_quantizer.fix_ranges()
    assert m.out_fixed8 is True                                                # active, frozen, asymmetric, 8 bits
    assert m.int8_index_ok(32) and not m.int8_index_ok(24)                     # (a call site's own extra condition: whole 16-row groups)
    m.full_precision_acts()
    assert not m.out_fixed8
    m.quantized_acts()
    m.activation_quantizer.estimate_ranges()
    assert not m.out_fixed8 and not m.int8_index_ok(32)
    for kw in (dict(act_method=Q.SymmetricUniformQuantizer), dict(n_bits_act=4)):
        m = _lin(**kw)
        m.quantized_acts()
        m.activation_quantizer.fix_ranges()
        assert m.activation_quantizer.is_fixed and not m.out_fixed8 and not m.int8_index_ok(32), kw
