"""The lean LDS-free kernels of csrc/ks_mlp.hip (kr_mlp3_forward_lean / kr_mlp3_backward_lean: tile pair (25, 19), the reference's
400-300) against a float64 reference, with the method and the helpers of tests/test_gpu_mlp_fp64.py: per layer from the kernel's
own stored activations, (a) bit-exact on dyadic inputs whose every partial sum is an fp32 number (asserted), (b) per-element
bounds (K + 4) * 2^-24 * (|W| |x| + |b|) on dense random inputs.  Then what is particular to these kernels: the partial last tiles
(392-292, and 300 = 18 * 16 + 12 itself) inside poisoned buffers, the refusals, mlp.supported(lean=True), and one learner update
on them (NativeDDPGfDUpdate(lean=True)) against float64 autograd."""
import pytest
import torch

from kinovagrasping_amd import mlp
from kinovagrasping_amd import sim as ks
from tests.test_gpu_mlp_fp64 import (DEV, KS_ERR_INVALID, SUPPORT_WIDTHS, U, _gen, _NoStep, _stream, assert_exact_ok, check_bound, check_exact,
                                     dense_net, dyadic, exact_net, lin, sigmoid_bound, to_dev, wide)

pytestmark = pytest.mark.gpu

WIDTHS = ((400, 300), (392, 292))          # the second: partial last tiles in both layers (392 = 24 * 16 + 8, 292 = 18 * 16 + 4)
NS = (1, 15, 16, 17, 33)                   # a partial row tile, an exact one, more than one wave
# (in_a, in_b, out_dim, act, scale, extra row stride of xa, of xb)
SHAPES = {"actor": (82, 0, 4, mlp.ACT_SIGMOID, 0.8, 18, 0), "critic": (82, 4, 1, mlp.ACT_NONE, 1.0, 3, 5)}


def _dev(t):
    return None if t is None else t.float().to(DEV).contiguous()


def run_forward(layers, xa, xb, act, scale, hid):
    n = xa.shape[0]
    (W1, _), (W2, _), _ = layers
    h1o = torch.full((n, W1.shape[0]), 7.0, device=DEV) if hid else None
    h2o = torch.full((n, W2.shape[0]), 7.0, device=DEV) if hid else None
    out = mlp.mlp3_forward(layers, xa, xb, act=act, scale=scale, h1_out=h1o, h2_out=h2o, lean=True)
    torch.cuda.synchronize()
    return out, h1o, h2o


def forward_exact(run, hw, in_a, in_b, out_dim, ea, eb, n, hid, g):
    h1, h2 = hw
    L, fx, (f1, f2, f3) = exact_net(h1, h2, in_a + in_b, out_dim, g)
    x = dyadic((n, in_a + in_b), fx, 3, 0.7, g)
    x[::5] = 0
    xa, xb = wide(x[:, :in_a], ea, g), (wide(x[:, in_a:], eb, g) if in_b else None)
    out, h1o, h2o = run(to_dev(L), xa, xb, mlp.ACT_NONE, 1.0, hid)
    (W1, b1), (W2, b2), (W3, b3) = L
    assert_exact_ok(x, W1.t(), b1, f1)
    z1 = x @ W1.t() + b1
    r1 = z1.clamp_min(0)
    assert (z1 == 0).any(), "no exactly-zero pre-activation"
    assert_exact_ok(r1, W2.t(), b2, f2)            # K = h1 = 400 / 392: the density rule of exact_net keeps it below 2^24 grid units
    r2 = (r1 @ W2.t() + b2).clamp_min(0)
    assert_exact_ok(r2, W3.t(), b3, f3)            # K = h2 = 300 / 292
    if hid:
        check_exact(h1o, r1, "h1 exact")
        check_exact(h2o, r2, "h2 exact")
    check_exact(out, r2 @ W3.t() + b3, "out exact")


@pytest.mark.parametrize("hid", [True, False], ids=["h", "noh"])
@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("hw", WIDTHS, ids=[f"{a}x{b}" for a, b in WIDTHS])
def test_forward_exact_and_bounded(hw, n, shape, hid):
    in_a, in_b, out_dim, act, scale, ea, eb = SHAPES[shape]
    in_dim, (h1, h2) = in_a + in_b, hw
    g = _gen("lean fwd", hw, n, shape, hid)
    forward_exact(run_forward, hw, in_a, in_b, out_dim, ea, eb, n, hid, g)                 # (a)
    L = dense_net(h1, h2, in_dim, out_dim, g)                                               # (b)
    x = torch.randn(n, in_dim, generator=g, dtype=torch.float64).float().double()
    xa, xb = wide(x[:, :in_a], ea, g), (wide(x[:, in_a:], eb, g) if in_b else None)
    out, h1o, h2o = run_forward(to_dev(L), xa, xb, act, scale, hid)
    (W1, b1), (W2, b2), (W3, b3) = L
    z1, m1 = lin(x, W1, b1)
    e1 = (in_dim + 4) * U * m1
    if hid:
        check_bound(h1o, z1.clamp_min(0), e1, "h1")
        z2, m2 = lin(h1o.double().cpu(), W2, b2)
        e2 = (h1 + 4) * U * m2
        check_bound(h2o, z2.clamp_min(0), e2, "h2")
        z3, m3 = lin(h2o.double().cpu(), W3, b3)
        e3 = (h2 + 4) * U * m3
    else:                                             # carried through the chain: |relu(a) - relu(b)| <= |a - b|
        r1 = z1.clamp_min(0)
        z2, m2 = lin(r1, W2, b2)
        e2 = e1 @ W2.abs().t() + (h1 + 4) * U * ((r1 + e1) @ W2.abs().t() + b2.abs())
        r2 = z2.clamp_min(0)
        z3, m3 = lin(r2, W3, b3)
        e3 = e2 @ W3.abs().t() + (h2 + 4) * U * ((r2 + e2) @ W3.abs().t() + b3.abs())
    if act == mlp.ACT_SIGMOID:
        a64 = scale * torch.sigmoid(z3)
        check_bound(out, a64, sigmoid_bound(z3, e3, scale, a64), "sigmoid out")
    else:
        check_bound(out, z3, e3, "out")


# ---- backward --------------------------------------------------------------------------------------------------------
def run_backward(layers, dz3, h1, h2, want, dxc, act_out, scale, scratch=None):
    """mlp.mlp3_backward when both or neither of dz2 / dz1 are wanted, the C ABI for one of them (or with the caller's scratch)"""
    (W1, _), (W2, _), (W3, _) = layers
    n = dz3.shape[0]
    if want[0] == want[1] and scratch is None:
        dz2, dz1, dx = mlp.mlp3_backward(layers, dz3, h1, h2, want_dz=want[0], dx_cols=None if dxc is None else dxc[1:], act_out=act_out, scale=scale,
                                         lean=True)
    else:
        lib, P = ks.load_library(), ks._ptr
        dz2 = torch.full_like(h2, 7.0) if want[0] else None
        dz1 = torch.full_like(h1, 7.0) if want[1] else None
        col0, ncol = (0, 0) if dxc is None else dxc[1:]
        dx = torch.full((n, ncol), 7.0, device=DEV) if dxc is not None else None
        if scratch is None:
            scratch = torch.full(((n + 15) // 16 * 16 * W2.shape[0],), float("nan"), device=DEV)       # whatever the memory held before
        rc = lib.kr_mlp3_backward_lean(n, W1.shape[1], W1.shape[0], W2.shape[0], W3.shape[0], P(dz3), P(W3), P(h2), P(W2), P(h1), P(dz2), P(dz1), P(W1),
                                       col0, ncol, P(act_out), float(scale), P(dx), P(scratch), scratch.numel(), _stream())
        assert rc == 0
    torch.cuda.synchronize()
    return dz2, dz1, dx


def backward_exact_inputs(hw, n, in_dim, out_dim, g):
    h1, h2 = hw
    d = lambda K: min(1.0, 24.0 / K)
    W1, W2, W3 = dyadic((h1, in_dim), 3, 3, d(h1), g), dyadic((h2, h1), 3, 3, d(h2), g), dyadic((out_dim, h2), 3, 3, 1.0, g)
    dz3 = dyadic((n, out_dim), 3, 3, 0.8, g)
    a1, a2 = dyadic((n, h1), 2, 3, 0.5, g, nonneg=True), dyadic((n, h2), 2, 3, 0.5, g, nonneg=True)   # stored activations, ~half zero
    return W1, W2, W3, dz3, a1, a2


def backward_exact_check(W1, W2, W3, dz3, a1, a2, dz2, dz1, dx, cols, act_out, scale):
    assert_exact_ok(dz3, W3, None, 6)
    r2 = (dz3 @ W3) * (a2 > 0)
    assert_exact_ok(r2, W2, None, 9)               # K = h2
    r1 = (r2 @ W2) * (a1 > 0)
    if dz2 is not None:
        check_exact(dz2, r2, "dz2 exact")
    if dz1 is not None:
        check_exact(dz1, r1, "dz1 exact")
    if cols is not None:
        assert_exact_ok(r1, W1[:, cols], None, 12)  # K = h1
        rx = r1 @ W1[:, cols]
        if act_out is not None:
            f = act_out * (1 - act_out / scale)
            assert float((rx.abs() * 2.0 ** 12 * f * 2.0 ** 8).max()) < 2.0 ** 24
            rx = rx * f
        check_exact(dx, rx, "dx exact")


# (out_dim, (in_dim, col0, ncol) of dx or None, sigmoid epilogue, (dz2_out given, dz1_out given))
BWD = {"actor-dz": (4, None, False, (True, True)), "actor-dz1": (4, None, False, (False, True)),
       "critic-dz-dx": (1, (86, 82, 4), True, (True, True)), "critic-dx": (1, (86, 82, 4), True, (False, False)),
       "critic-dz2-dx-lin": (1, (86, 82, 4), False, (True, False))}


@pytest.mark.parametrize("kind", list(BWD))
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("hw", WIDTHS, ids=[f"{a}x{b}" for a, b in WIDTHS])
def test_backward_exact_and_bounded(hw, n, kind):
    out_dim, dxc, act, want = BWD[kind]
    h1, h2 = hw
    in_dim = dxc[0] if dxc else 82
    g = _gen("lean bwd", hw, n, kind)
    cols = slice(dxc[1], dxc[1] + dxc[2]) if dxc else None
    # (a) exact; the sigmoid epilogue with a power-of-two scale (a / scale, 1 - a / scale, a (1 - a / scale) exact)
    W1, W2, W3, dz3, a1, a2 = backward_exact_inputs(hw, n, in_dim, out_dim, g)
    scale = 0.5
    act_out = (torch.randint(1, 8, (n, dxc[2]), generator=g).double() * 2.0 ** -4) if act else None     # in (0, scale)
    layers = [(_dev(W1), None), (_dev(W2), None), (_dev(W3), None)]
    dz2, dz1, dx = run_backward(layers, _dev(dz3), _dev(a1), _dev(a2), want, dxc, _dev(act_out), scale)
    backward_exact_check(W1, W2, W3, dz3, a1, a2, dz2 if want[0] else None, dz1 if want[1] else None, dx, cols, act_out, scale)
    # (b) dense: the bounds of tests/test_gpu_mlp_fp64.py::test_backward_exact_and_bounded
    scale = 0.8
    (W1, _), (W2, _), (W3, _) = dense_net(h1, h2, in_dim, out_dim, g)
    dz3 = torch.randn(n, out_dim, generator=g, dtype=torch.float64).float().double()
    a1 = torch.randn(n, h1, generator=g, dtype=torch.float64).float().double().clamp_min(0)
    a2 = torch.randn(n, h2, generator=g, dtype=torch.float64).float().double().clamp_min(0)
    act_out = (scale * torch.sigmoid(torch.randn(n, dxc[2], generator=g, dtype=torch.float64))).float().double() if act else None
    layers = [(_dev(W1), None), (_dev(W2), None), (_dev(W3), None)]
    dz2, dz1, dx = run_backward(layers, _dev(dz3), _dev(a1), _dev(a2), want, dxc, _dev(act_out), scale)
    m2 = a2 > 0
    r2 = (dz3 @ W3) * m2
    e2 = (out_dim + 4) * U * (dz3.abs() @ W3.abs()) * m2
    if want[0]:
        check_bound(dz2, r2, e2, "dz2")
        r2, e2 = dz2.double().cpu(), torch.zeros_like(e2)
    m1 = a1 > 0
    r1 = (r2 @ W2) * m1
    e1 = ((h2 + 4) * U * ((r2.abs() + e2) @ W2.abs()) + e2 @ W2.abs()) * m1
    if want[1]:
        check_bound(dz1, r1, e1, "dz1")
        r1, e1 = dz1.double().cpu(), torch.zeros_like(e1)
    if dxc:
        Wc = W1[:, cols]
        v = r1 @ Wc
        ev = (h1 + 4) * U * ((r1.abs() + e1) @ Wc.abs()) + e1 @ Wc.abs()
        if act:
            f = act_out * (1 - act_out / scale)
            ef = (act_out.abs() * (act_out / scale).abs() + 3 * f.abs()) * U
            check_bound(dx, v * f, (v.abs() + ev) * (f.abs() + ef) * U + ev * (f.abs() + ef) + v.abs() * ef, "dx sigmoid epilogue")
        else:
            check_bound(dx, v, ev, "dx")


# ---- (c) the partial tiles inside poisoned buffers ---------------------------------------------------------------------
POISON, PAD = 1e30, 64                     # PAD floats (a multiple of 4: 16-byte alignment is kept) on either side


class Embedded:
    """a tensor in the middle of a larger buffer whose surroundings hold POISON"""

    def __init__(self, t, fill=None):
        self.buf = torch.full((t.numel() + 2 * PAD,), POISON, device=DEV)
        self.t = self.buf[PAD:PAD + t.numel()].view(t.shape)
        self.t.copy_(t.float() if fill is None else torch.full_like(self.t, fill))

    def surroundings_intact(self):
        return bool((self.buf[:PAD] == POISON).all() and (self.buf[-PAD:] == POISON).all())


@pytest.mark.parametrize("hw", WIDTHS, ids=[f"{a}x{b}" for a, b in WIDTHS])
def test_partial_tiles_neither_read_nor_write_their_surroundings(hw):
    """Weights, biases and the hidden outputs sit between stretches of 1e30; W3 has a second output row, so that a read past the
    last column of row 0 would land in real data (and one past the last row in poison); the scratch buffers hold NaN.  On dyadic
    inputs the results still equal the fp64 reference in every bit, and no poisoned word has changed."""
    lib, P = ks.load_library(), ks._ptr
    h1, h2 = hw
    n, in_a, in_b, out_dim = 17, 82, 4, 2
    g = _gen("lean poison", hw)
    L, fx, (f1, f2, f3) = exact_net(h1, h2, in_a + in_b, out_dim, g)
    x = dyadic((n, in_a + in_b), fx, 3, 0.7, g)
    xa, xb = wide(x[:, :in_a], 3, g), wide(x[:, in_a:], 5, g)
    (W1, b1), (W2, b2), (W3, b3) = L
    e = {k: Embedded(v) for k, v in (("W1", W1), ("b1", b1), ("W2", W2), ("b2", b2), ("W3", W3), ("b3", b3))}
    outs = {k: Embedded(torch.empty(s), fill=7.0) for k, s in (("h1", (n, h1)), ("h2", (n, h2)), ("out", (n, out_dim)))}
    for keep_h1 in (True, False):
        for v in outs.values():
            v.t.fill_(7.0)
        scratch = torch.full(((n + 15) // 16 * 16 * h1,), float("nan"), device=DEV)
        rc = lib.kr_mlp3_forward_lean(n, in_a, in_b, h1, h2, out_dim, P(xa), xa.stride(0), P(xb), xb.stride(0), P(e["W1"].t), P(e["b1"].t), P(e["W2"].t),
                                      P(e["b2"].t), P(e["W3"].t), P(e["b3"].t), mlp.ACT_NONE, 1.0, P(outs["out"].t), P(outs["h1"].t) if keep_h1 else None,
                                      P(outs["h2"].t), None if keep_h1 else P(scratch), 0 if keep_h1 else scratch.numel(), _stream())
        torch.cuda.synchronize()
        assert rc == 0
        assert_exact_ok(x, W1.t(), b1, f1)
        r1 = (x @ W1.t() + b1).clamp_min(0)
        assert_exact_ok(r1, W2.t(), b2, f2)
        r2 = (r1 @ W2.t() + b2).clamp_min(0)
        assert_exact_ok(r2, W3.t(), b3, f3)
        if keep_h1:
            check_exact(outs["h1"].t, r1, "h1 exact")
        else:
            assert (outs["h1"].t == 7.0).all()
        check_exact(outs["h2"].t, r2, "h2 exact")
        check_exact(outs["out"].t, r2 @ W3.t() + b3, "out exact")
        assert all(v.surroundings_intact() for v in list(e.values()) + list(outs.values()))
    # backward: the same arrangement for W1 .. W3, the stored activations and dz2 / dz1 / dx
    W1, W2, W3, dz3, a1, a2 = backward_exact_inputs(hw, n, in_a + in_b, out_dim, g)
    e = {k: Embedded(v) for k, v in (("W1", W1), ("W2", W2), ("W3", W3), ("a1", a1), ("a2", a2), ("dz3", dz3))}
    outs = {k: Embedded(torch.empty(s), fill=7.0) for k, s in (("dz2", (n, h2)), ("dz1", (n, h1)), ("dx", (n, 4)))}
    for keep_dz2 in (True, False):
        for v in outs.values():
            v.t.fill_(7.0)
        scratch = torch.full(((n + 15) // 16 * 16 * h2,), float("nan"), device=DEV)
        rc = lib.kr_mlp3_backward_lean(n, in_a + in_b, h1, h2, out_dim, P(e["dz3"].t), P(e["W3"].t), P(e["a2"].t), P(e["W2"].t), P(e["a1"].t),
                                       P(outs["dz2"].t) if keep_dz2 else None, P(outs["dz1"].t), P(e["W1"].t), in_a, in_b, None, 1.0, P(outs["dx"].t),
                                       None if keep_dz2 else P(scratch), 0 if keep_dz2 else scratch.numel(), _stream())
        torch.cuda.synchronize()
        assert rc == 0
        assert keep_dz2 or (outs["dz2"].t == 7.0).all()
        backward_exact_check(W1, W2, W3, dz3, a1, a2, outs["dz2"].t if keep_dz2 else None, outs["dz1"].t, outs["dx"].t, slice(in_a, in_a + in_b), None, 1.0)
        assert all(v.surroundings_intact() for v in list(e.values()) + list(outs.values()))


# ---- (d) refusals ----------------------------------------------------------------------------------------------------
FWD_REFUSALS = {
    # (in_a, in_b, widths, out_dim, misaligned h1_out, keep h1, scratch: "ok" / "null" / "short")
    "256x256": (82, 4, (256, 256), 1, False, True, "ok"),
    "398x298": (82, 4, (398, 298), 1, False, False, "ok"),
    "in97": (93, 4, (400, 300), 1, False, True, "ok"),
    "out5": (82, 0, (400, 300), 5, False, True, "ok"),
    "misaligned-h1_out": (82, 0, (400, 300), 4, True, True, "ok"),
    "scratch-null": (82, 0, (400, 300), 4, False, False, "null"),
    "scratch-short": (82, 0, (400, 300), 4, False, False, "short"),
}


@pytest.mark.parametrize("case", list(FWD_REFUSALS))
def test_forward_refusals_leave_the_outputs_alone(case):
    in_a, in_b, (h1, h2), out_dim, mis, keep_h1, scr = FWD_REFUSALS[case]
    lib, P = ks.load_library(), ks._ptr
    n = 17
    in_dim = in_a + in_b
    W = [torch.randn(h1, in_dim, device=DEV), torch.randn(h1, device=DEV), torch.randn(h2, h1, device=DEV), torch.randn(h2, device=DEV),
         torch.randn(out_dim, h2, device=DEV), torch.randn(out_dim, device=DEV)]
    xa, xb = torch.randn(n, in_a, device=DEV), (torch.randn(n, in_b, device=DEV) if in_b else None)
    out = torch.full((n, out_dim), 12345.0, device=DEV)
    h1buf = torch.full((n * h1 + 4,), 12345.0, device=DEV)
    h1o = (h1buf[1:1 + n * h1] if mis else h1buf[:n * h1]) if keep_h1 else None
    h2o = torch.full((n, h2), 12345.0, device=DEV)
    need = (n + 15) // 16 * 16 * h1
    scratch = torch.full((need,), 12345.0, device=DEV)
    rc = lib.kr_mlp3_forward_lean(n, in_a, in_b, h1, h2, out_dim, P(xa), in_a, P(xb), in_b, *(P(w) for w in W), mlp.ACT_NONE, 1.0, P(out), P(h1o), P(h2o),
                                  None if scr == "null" else P(scratch), need - 1 if scr == "short" else need, _stream())
    torch.cuda.synchronize()
    assert rc == KS_ERR_INVALID
    assert (out == 12345.0).all() and (h1buf == 12345.0).all() and (h2o == 12345.0).all() and (scratch == 12345.0).all()


BWD_REFUSALS = {
    # (widths, out_dim, misaligned dz1_out, keep dz2, (col0, ncol), scratch)
    "256x256": ((256, 256), 1, False, True, (82, 4), "ok"),
    "398x298": ((398, 298), 1, False, False, (82, 4), "ok"),
    "out5": ((400, 300), 5, False, True, (82, 4), "ok"),
    "misaligned-dz1_out": ((400, 300), 1, True, True, (82, 4), "ok"),
    "dx-past-in_dim": ((400, 300), 1, False, True, (84, 4), "ok"),
    "scratch-null": ((400, 300), 1, False, False, (82, 4), "null"),
    "scratch-short": ((400, 300), 1, False, False, (82, 4), "short"),
}


@pytest.mark.parametrize("case", list(BWD_REFUSALS))
def test_backward_refusals_leave_the_outputs_alone(case):
    (h1, h2), out_dim, mis, keep_dz2, dxc, scr = BWD_REFUSALS[case]
    lib, P = ks.load_library(), ks._ptr
    n, in_dim = 17, 86
    W1, W2, W3 = torch.randn(h1, in_dim, device=DEV), torch.randn(h2, h1, device=DEV), torch.randn(out_dim, h2, device=DEV)
    dz3, a1, a2 = torch.randn(n, out_dim, device=DEV), torch.rand(n, h1, device=DEV), torch.rand(n, h2, device=DEV)
    dz2 = torch.full((n, h2), 12345.0, device=DEV)
    dz1buf = torch.full((n * h1 + 4,), 12345.0, device=DEV)
    dz1 = dz1buf[1:1 + n * h1] if mis else dz1buf[:n * h1]
    dx = torch.full((n, 4), 12345.0, device=DEV)
    need = (n + 15) // 16 * 16 * h2
    scratch = torch.full((need,), 12345.0, device=DEV)
    rc = lib.kr_mlp3_backward_lean(n, in_dim, h1, h2, out_dim, P(dz3), P(W3), P(a2), P(W2), P(a1), P(dz2) if keep_dz2 else None, P(dz1), P(W1), dxc[0], dxc[1],
                                   None, 1.0, P(dx), None if scr == "null" else P(scratch), need - 1 if scr == "short" else need, _stream())
    torch.cuda.synchronize()
    assert rc == KS_ERR_INVALID
    assert (dz2 == 12345.0).all() and (dz1buf == 12345.0).all() and (dx == 12345.0).all() and (scratch == 12345.0).all()


# ---- (e) mlp.supported(lean=True) ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", SUPPORT_WIDTHS, ids=[f"{h[0]}x{h[1]}" for h in SUPPORT_WIDTHS])
def test_supported_lean_says_exactly_when_the_launch_runs(hw):
    lib, P = ks.load_library(), ks._ptr
    n = 17
    assert mlp.LEAN_TILES == {(25, 19)}
    for in_a, in_b, out_dim in ((82, 0, 4), (82, 4, 1), (92, 4, 1), (93, 4, 1)):
        layers = [(torch.randn(o, i, device=DEV) * 0.1, torch.zeros(o, device=DEV)) for o, i in ((hw[0], in_a + in_b), (hw[1], hw[0]), (out_dim, hw[1]))]
        (W1, b1), (W2, b2), (W3, b3) = layers
        xa, xb = torch.randn(n, in_a, device=DEV), (torch.randn(n, in_b, device=DEV) if in_b else None)
        out = torch.empty(n, out_dim, device=DEV)
        need = (n + 15) // 16 * 16 * hw[0]
        scratch = torch.empty(need, device=DEV)
        rc = lib.kr_mlp3_forward_lean(n, in_a, in_b, hw[0], hw[1], out_dim, P(xa), in_a, P(xb), in_b, P(W1), P(b1), P(W2), P(b2), P(W3), P(b3), mlp.ACT_NONE,
                                      1.0, P(out), None, None, P(scratch), need, _stream())
        torch.cuda.synchronize()
        assert rc in (0, KS_ERR_INVALID)
        assert mlp.supported(layers, in_a + in_b, lean=True) == (rc == 0), (hw, in_a + in_b, rc)


# ---- (f) one learner update ------------------------------------------------------------------------------------------------
def test_lean_learner_update_against_fp64_autograd():
    """NativeDDPGfDUpdate(policy, lean=True) at 400-300 - every pass on the lean kernels and kr_weight_grad_shadow - with the batch and
    the criterion of tests/test_gpu_mlp_fp64.py::test_learner_update_against_fp64_autograd: per tensor, the native error is at most
    4 x that of fp32 torch autograd on the same data, or 1e-6 of the tensor's largest entry.  R = 37 masked rows, n = 5."""
    from kinovagrasping_amd.ddpgfd import DDPGfD
    from kinovagrasping_amd.learner_native import NativeDDPGfDUpdate
    hidden = (400, 300)

    def make():
        torch.manual_seed(7)
        return DDPGfD(82, 4, 0.8, 5, hidden=hidden, device=DEV)

    default = NativeDDPGfDUpdate(make())
    assert default.lds_free is False and not default.lean                  # nothing that runs today changes form
    p32, pn, p64 = make(), make(), make()
    for name in ("actor", "critic", "actor_target", "critic_target"):
        getattr(p64, name).double()
    p64._disc = p64._disc.double()
    nat = NativeDDPGfDUpdate(pn, lean=True)
    assert nat.lean and nat.lds_free and nat.lean_kernels
    with pytest.raises(ValueError):
        torch.manual_seed(7)
        NativeDDPGfDUpdate(DDPGfD(82, 4, 0.8, 5, hidden=(200, 100), device=DEV), lean=True)
    g = torch.Generator(device=DEV).manual_seed(11)
    R, n = 37, 5
    st = torch.randn(R, n, 82, device=DEV, generator=g) * 0.3
    ns = torch.randn(R, n, 82, device=DEV, generator=g) * 0.3
    ac = torch.rand(R, n, 4, device=DEV, generator=g) * 0.8
    rw = torch.rand(R, n, device=DEV, generator=g) * 5
    w = (torch.rand(R, device=DEV, generator=g) < 0.7).float()
    w[:3] = 0
    w[3] = 1
    assert 0 < w.sum().item() < R

    def compare(native, t32, t64, what):
        for k, (a, b, c) in enumerate(zip(native, t32, t64)):
            a, b, c = a.double(), b.double(), c.double()
            e_nat, e_32 = (a - c).abs().max().item(), (b - c).abs().max().item()
            print(f"{what}[{k}]: native error {e_nat:.3g}, fp32 autograd error {e_32:.3g}, largest entry {c.abs().max().item():.3g}")
            assert e_nat <= max(4 * e_32, 1e-6 * c.abs().max().item()), (what, k, e_nat, e_32, c.abs().max().item())

    l32 = p32.phase_critic(st, ac, ns, rw, w)
    l64 = p64.phase_critic(st.double(), ac.double(), ns.double(), rw.double(), w.double())
    ln = nat.phase_critic(st, ac, ns, rw, w)
    torch.cuda.synchronize()
    compare([x.reshape(1) for x in ln], [x.reshape(1) for x in l32], [x.reshape(1) for x in l64], "critic losses")
    grads = lambda m: [p.grad for p in m.parameters()]
    nat_grads = lambda net: [t for pair in zip(net.gW, net.gb) for t in pair]
    compare(nat_grads(nat.critic), grads(p32.critic), grads(p64.critic), "critic gradient")
    # actor phase: the reference critic takes the native critic's parameters after its Adam step
    nat.phase_actor(st, w)
    torch.cuda.synchronize()
    p32._flat_params["critic"].copy_(nat.critic.flat)
    for q, src in zip(p64.critic.parameters(), pn.critic.parameters()):
        q.data.copy_(src.data.double())
    p32.critic_optimizer, p64.critic_optimizer = _NoStep(), _NoStep()
    p32.phase_actor(st, w)
    p64.phase_actor(st.double(), w.double())
    compare(nat_grads(nat.actor), grads(p32.actor), grads(p64.actor), "actor gradient")
