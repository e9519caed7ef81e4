"""tests/derived_state.py has teeth: on a stand-in engine of CPU tensors -- a 3x3 conv with 32 input channels as F(4x4,3x3), a second
one as F(2x2,3x3), a 1x1 conv with a ragged pitch (20 of 24 columns, its shift the bias itself, like rpn_heads) and a layer whose n = 12 is
no multiple of 8 -- a state computed the way the kernels compute it (fp32, the kernels' association) audits clean, and each of seven stale
or misplaced copies is flagged on exactly its own record: a shift from biases one Adam step old, a U from the old kernel, a U in the other
form, one bf16 element one unit in the last place off, one nonzero padding element, a dgrad image laid out tap-minor, a forward image that
was not transposed.  A buffer excused by _inference_filters_stale is reported as excused, and audit(inference=True) has it rewritten."""
import collections
import types

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import derived_state as D  # noqa: E402
import winograd_edge_cases as W  # noqa: E402

LR = 2e-5
FwdImage = collections.namedtuple("FwdImage", "wt ldk conv n")
DgradImage = collections.namedtuple("DgradImage", "wd ldkd conv n")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _shift(c):
    return (c.scale.numpy() * c.bias.numpy() + c.t0.numpy()).astype(np.float32) if c.t0 is not None else None


def _u(c, w=None, form=None):
    form = form or c.wino_m
    w = c.weight.numpy() if w is None else w
    res = W.stage_filter(w, c.cin, c.cout, c.ldw, form, arith="kernel")
    return res["buf"][:(form + 2) ** 2 * c.cin * c.cout].astype(np.float32).reshape((form + 2) ** 2, c.cin, c.cout)


def _fwd(c, n):
    k = c.kh * c.kh * c.cin
    ldk = (k + 31) // 32 * 32
    return FwdImage(_t(D.fwd_image_ref(c.weight.numpy(), k, n, ldk).view(np.int16)), ldk, c, n)


def _dgrad(c, n):
    taps = c.kh * c.kh
    ldkd = (taps * ((n + 7) // 8 * 8) + 31) // 32 * 32
    return DgradImage(_t(D.dgrad_image_ref(c.weight.numpy(), taps, c.cin, n, ldkd).view(np.int16)), ldkd, c, n)


class StandIn:
    INFERENCE_WINOGRAD_LAYERS = ("b3x3",)

    def __init__(self):
        rs = np.random.RandomState(11)
        self.convs = collections.OrderedDict()
        for name, kh, cin, cout, ldw, form, fold in (("a3x3", 3, 32, 16, 16, 4, True), ("b3x3", 3, 32, 8, 12, 2, True),
                                                     ("heads", 1, 32, 20, 24, 0, False), ("odd_n", 1, 16, 12, 12, 0, True)):
            c = types.SimpleNamespace(name=name, kh=kh, cin=cin, cout=cout, ldw=ldw, wino_u=None, wino_m=form or 2)
            c.weight = _t(rs.standard_normal((kh * kh * cin, ldw)).astype(np.float32))
            nb = cout if fold else ldw
            c.bias = _t(rs.standard_normal(nb).astype(np.float32))
            c.scale = _t(rs.uniform(0.5, 1.5, nb).astype(np.float32)) if fold else None
            c.t0 = _t(rs.standard_normal(nb).astype(np.float32)) if fold else None
            c.shift = _t(_shift(c)) if fold else c.bias
            if form:
                c.wino_u = _t(_u(c))
            self.convs[name] = c
        self.bf16 = types.SimpleNamespace(fwd={}, dgrad={})
        for k, c in enumerate(self.convs.values()):
            self.bf16.fwd[k] = _fwd(c, c.cout)
            self.bf16.dgrad[k] = _dgrad(c, c.cout)
        self._inference_filters_stale = False
        self.synced = 0

    def sync_inference_filters(self):
        self.synced += 1
        if self._inference_filters_stale:
            self._inference_filters_stale = False
            c = self.convs["b3x3"]
            c.wino_u = _t(_u(c))
            for k, cc in enumerate(self.convs.values()):
                self.bf16.fwd[k] = _fwd(cc, cc.cout)
                self.bf16.dgrad[k] = _dgrad(cc, cc.cout)

    def image(self, table, layer):
        k = list(self.convs).index(layer)
        return k, getattr(self.bf16, table)[k]


def _flagged(eng, **kw):
    return sorted((r.layer, r.kind) for r in D.wrong(D.audit(eng, **kw)))


def test_the_two_bf16_statements_agree_on_ties_subnormals_and_both_signs():
    rs = np.random.RandomState(0)
    w = (rs.randn(64, 8) * 10.0 ** rs.uniform(-30, 30, (64, 8))).astype(np.float32)
    bits = w.view(np.uint32)
    bits[0:8] = (rs.randint(0x3f80, 0x4f80, (8, 8)).astype(np.uint32) << 16) | 0x8000 | (rs.randint(0, 2, (8, 8)).astype(np.uint32) << 31)
    bits[8:12] = rs.randint(1, 0x7fffff, (4, 8)).astype(np.uint32)
    assert np.array_equal(D.fwd_image_bits(w, 8), D.bf16_bits(w).T)


def test_a_state_the_kernels_would_compute_audits_clean_and_every_buffer_has_a_record():
    eng = StandIn()
    rec = D.audit(eng)
    assert sorted((r.layer, r.kind) for r in rec) == sorted(
        [(n, "shift") for n in eng.convs] + [("a3x3", "wino_u"), ("b3x3", "wino_u")] + [(n, k) for n in eng.convs for k in ("bf16_fwd", "bf16_dgrad")])
    assert D.wrong(rec) == [] and not any(r.excused for r in rec)
    for r in rec:
        assert r.n_wrong == 0 and r.worst <= 1.0, r
        if r.kind in ("shift", "wino_u") and r.layer != "heads":
            assert r.worst > 0, r                      # fp32 against float64: the rounding is there, inside its bound
    assert eng.synced == 0
    D.assert_clean(rec)
    assert [(r.layer, r.kind) for r in D.audit(eng, kinds=("wino_u",), layers=("b3x3",))] == [("b3x3", "wino_u")]


def test_a_shift_that_lags_one_adam_step_is_flagged():
    for layer in ("a3x3", "odd_n"):
        eng = StandIn()
        c = eng.convs[layer]
        old = types.SimpleNamespace(scale=c.scale, t0=c.t0, bias=_t(c.bias.numpy() - np.float32(LR)))
        c.shift = _t(_shift(old))
        assert _flagged(eng) == [(layer, "shift")]
        r = [r for r in D.audit(eng) if (r.layer, r.kind) == (layer, "shift")][0]
        assert r.n_wrong == c.cout and r.worst > 20, r          # lr * scale against 2^-23 * (|scale * bias| + |t0|): not a near miss
    eng = StandIn()                                             # without a fold the shift is the bias, bit for bit
    c = eng.convs["heads"]
    c.shift = c.bias.clone()
    assert _flagged(eng) == []
    c.shift[3] += LR
    assert _flagged(eng) == [("heads", "shift")]


def test_a_u_from_the_old_kernel_and_a_u_in_the_other_form_are_flagged():
    for layer in ("a3x3", "b3x3"):
        eng = StandIn()
        c = eng.convs[layer]
        rs = np.random.RandomState(5)
        c.wino_u = _t(_u(c, c.weight.numpy() - np.float32(LR) * np.sign(rs.standard_normal(tuple(c.weight.shape))).astype(np.float32)))
        assert _flagged(eng) == [(layer, "wino_u")]
        eng = StandIn()
        c = eng.convs[layer]
        c.wino_u = _t(_u(c, form=6 - c.wino_m))                  # F(2x2) filters where the layer says F(4x4), and the reverse
        assert _flagged(eng) == [(layer, "wino_u")]
        eng = StandIn()
        eng.convs[layer].wino_m = 6 - eng.convs[layer].wino_m    # ... or the form changed and the filters stayed
        assert _flagged(eng) == [(layer, "wino_u")]


@pytest.mark.parametrize("table", ["fwd", "dgrad"])
def test_one_bf16_unit_and_one_padding_element_are_flagged(table):
    kind = "bf16_" + table
    for layer, at in (("a3x3", (3, 5)), ("heads", (7, 1)), ("odd_n", (11, 0))):
        eng = StandIn()
        _, im = eng.image(table, layer)
        im[0][at] += 1                                           # one unit in the last place
        assert _flagged(eng) == [(layer, kind)]
        assert [r.n_wrong for r in D.audit(eng) if (r.layer, r.kind) == (layer, kind)] == [1]
    # padding: columns K .. ldk of a forward image (K = 16 of 32), columns n .. n8 and taps * n8 .. ldkd of a dgrad image (n = 12 of 16, 16 of 32)
    for layer, at in ((("odd_n", (2, 19)),) if table == "fwd" else (("odd_n", (2, 13)), ("odd_n", (5, 31)), ("heads", (0, 21)))):
        eng = StandIn()
        _, im = eng.image(table, layer)
        assert im[0][at] == 0
        im[0][at] = 1
        assert _flagged(eng) == [(layer, kind)]


def test_a_dgrad_image_laid_out_tap_minor_is_flagged():
    eng = StandIn()
    k, im = eng.image("dgrad", "a3x3")
    c, taps = im.conv, 9
    b = D.bf16_bits(c.weight.numpy()[:, :im.n]).reshape(taps, c.cin, im.n)
    wd = np.zeros((c.cin, im.ldkd), np.uint16)
    for t in range(taps):
        wd[:, t:taps * im.n:taps] = b[t]                         # element j * taps + t
    eng.bf16.dgrad[k] = im._replace(wd=_t(wd.view(np.int16)))
    assert _flagged(eng) == [("a3x3", "bf16_dgrad")]


def test_a_forward_image_that_was_not_transposed_is_flagged():
    for layer in ("a3x3", "odd_n"):
        eng = StandIn()
        k, im = eng.image("fwd", layer)
        c = im.conv
        kk = c.kh * c.kh * c.cin
        wt = np.zeros((im.n, im.ldk), np.uint16)
        wt[:, :kk] = D.bf16_bits(c.weight.numpy()[:, :im.n]).reshape(im.n, kk)          # [K][n] read as [n][K]
        eng.bf16.fwd[k] = im._replace(wt=_t(wt.view(np.int16)))
        assert _flagged(eng) == [(layer, "bf16_fwd")]


def test_what_the_stale_flag_excuses_is_reported_as_excused_and_inference_has_it_rewritten():
    eng = StandIn()
    for c in eng.convs.values():                                 # other weights were loaded (a step of lr moves few bf16 values); nothing was rewritten
        c.weight = _t(c.weight.numpy() + np.float32(0.01))
    eng._inference_filters_stale = True
    rec = D.audit(eng)
    assert _flagged(eng) == [("a3x3", "wino_u")]                 # a training-path buffer: no excuse
    excused = sorted((r.layer, r.kind) for r in rec if r.excused)
    assert ("b3x3", "wino_u") in excused and ("a3x3", "bf16_fwd") in excused and ("odd_n", "bf16_dgrad") in excused
    assert all(r.n_wrong > 0 for r in rec if r.excused)          # the figures stay
    assert eng.synced == 0
    assert _flagged(eng, inference=True) == [("a3x3", "wino_u")] and eng.synced == 1
    assert not any(r.excused for r in D.audit(eng))
    eng._inference_filters_stale = False                         # without the flag the same lag is an error
    c = eng.convs["b3x3"]
    c.weight = _t(c.weight.numpy() + np.float32(0.01))
    assert ("b3x3", "wino_u") in _flagged(eng) and ("b3x3", "bf16_fwd") in _flagged(eng)
