"""The actor / critic kernels of csrc/ks_mlp.hip against a float64 reference of the same operation, at every instantiated width.

Every entry point is called through mlp.py where it exposes the form and the argument, through the C ABI otherwise.  The
reference is torch float64 on the host, from the same fp32 parameters and inputs, and each layer is checked on its own: the
layer-2 reference takes the kernel's own h1_out, layer 3 its h2_out, the backward the stored activations (a ReLU boundary
flip cannot compound and hide an error).  Two checks per case:

  (a) exact: dyadic inputs (small integers times 2^-k, many zeros) on which every partial sum of every reduction is an fp32
      number - asserted per element: sum |terms| * 2^f < 2^24 on the grid 2^-f.  Any summation order is then exact (the f32
      MFMA is bitwise a k-ordered fmaf chain), so the kernel equals the fp64 reference in every bit: a dropped, duplicated or
      misplaced term of any size shows.  Pre-activations that are exactly 0 exercise the ReLU's h > 0 branch.
  (b) dense random: |y - y64| <= (K + 4) * 2^-24 * (|W| |x| + |b|) per element, K = that element's reduction length.  Where
      a hidden layer is not returned the bound is carried through the chain (ReLU is 1-Lipschitz).  Sigmoid outputs
      (scale / (1 + __expf(-z)), fast exp with a relative error that grows with |z|) add
      s'(z) * scale * ((|z| + 4) * 2^-24 + bound(z)) + 2 ulp(a), s' taken at the point of z's interval nearest 0.

Then one DDPGfD learner update per form (learner_native) against float64 autograd of DDPGfD's own losses.
"""
import ctypes
import zlib

import pytest
import torch

from kinovagrasping_amd import mlp
from kinovagrasping_amd import sim as ks

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
NS = (1, 15, 16, 17, 63, 64, 65, 4097)
NOMINAL = ((256, 256), (400, 300), (128, 128), (64, 64))
LDS_FREE = ((256, 256), (128, 128), (64, 64))
KS_ERR_INVALID = -1
DEV = torch.device("cuda", 0)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


# ---- inputs ----------------------------------------------------------------------------------------------------------
def dyadic(shape, k, vmax, density, g, nonneg=False):
    """integers in [-vmax, vmax] ([0, vmax] if nonneg) times 2^-k, each nonzero with probability `density` (fp64, exact in fp32)"""
    v = torch.randint(0 if nonneg else -vmax, vmax + 1, shape, generator=g).double()
    v[torch.rand(shape, generator=g) >= density] = 0
    return v * 2.0 ** -k


def on_grid(t, f):
    s = t * 2.0 ** f
    return bool((s == s.round()).all())


def assert_exact_ok(a, b, c, f):
    """precondition of bit-equality for  y = a @ b (+ c):  a @ b and c on the grid 2^-f, sum |terms| * 2^f < 2^24 per element"""
    mag = a.abs() @ b.abs() + (0 if c is None else c.abs())
    assert float(mag.max()) * 2.0 ** f < 2.0 ** 24, "dyadic inputs too large for an exact fp32 reduction"
    assert c is None or on_grid(c, f)


def exact_net(h1, h2, in_dim, out_dim, g, with_zero_units=True):
    """dyadic layers: W on 2^-3, biases on the grid of their layer's products; density ~ 24 nonzero terms per output so that
    three layers of products stay below 2^24 grid units.  Returns [(W, b)] fp64 and the grids of the three layers' outputs."""
    fx = 2
    d = lambda K: min(1.0, 24.0 / K)
    W1, W2, W3 = dyadic((h1, in_dim), 3, 3, d(in_dim), g), dyadic((h2, h1), 3, 3, d(h1), g), dyadic((out_dim, h2), 3, 3, d(h2), g)
    f1, f2, f3 = fx + 3, fx + 6, fx + 9
    b1, b2, b3 = dyadic((h1,), 1, 3, 0.5, g), dyadic((h2,), 4, 3, 0.5, g), dyadic((out_dim,), 7, 3, 0.5, g)
    if with_zero_units:
        b1[:4] = 0
    return [(W1, b1), (W2, b2), (W3, b3)], fx, (f1, f2, f3)


def dense_net(h1, h2, in_dim, out_dim, g):
    """torch.nn.Linear-like initialisation with biases that put about half of the ReLUs on"""
    out = []
    for o, i in ((h1, in_dim), (h2, h1), (out_dim, h2)):
        out.append((torch.randn(o, i, generator=g, dtype=torch.float64).float().double() / i ** 0.5,
                    (0.1 * torch.randn(o, generator=g, dtype=torch.float64)).float().double()))
    return out


def to_dev(layers):
    return [(W.float().to(DEV).contiguous(), b.float().to(DEV).contiguous()) for W, b in layers]


def wide(x, extra, g):
    """x [n, k] as a row-strided view (row stride k + extra) of a wider device tensor, the padding filled with garbage"""
    n, k = x.shape
    buf = torch.randn(n, k + extra, generator=g) * 1e3
    buf[:, :k] = x.float()
    buf = buf.to(DEV)
    return buf[:, :k]


# ---- fp64 reference and bounds ---------------------------------------------------------------------------------------
def lin(x, W, b):
    """z = x W^T + b and its rounding scale |x| |W|^T + |b|"""
    return x @ W.t() + (0 if b is None else b), x.abs() @ W.abs().t() + (0 if b is None else b.abs())


def ulp32(a):
    a = a.abs().float().clamp_min(torch.finfo(torch.float32).tiny)
    return (torch.nextafter(a, torch.full_like(a, float("inf"))) - a).double()


def sigmoid_bound(z, ez, scale, a64):
    """bound of |scale / (1 + __expf(-z~)) - scale * sigmoid(z)| for |z~ - z| <= ez (module docstring)"""
    zc = torch.where((z - ez <= 0) & (z + ez >= 0), torch.zeros_like(z), torch.where(z > 0, z - ez, z + ez))
    sc = torch.sigmoid(zc)
    return sc * (1 - sc) * scale * ((z.abs() + ez + 4) * U + ez) + 2 * ulp32(a64)


def check_exact(got, ref, what):
    got = got.double().cpu()
    bad = (got != ref)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.numel()} elements differ from the exact result, first at {bad.nonzero()[0].tolist()}"


def check_bound(got, ref, bound, what):
    got = got.double().cpu()
    err = (got - ref).abs()
    bad = ~(err <= bound)
    assert not bad.any(), (f"{what}: {int(bad.sum())} of {bad.numel()} elements outside the bound, worst err / bound "
                           f"{float((err / bound.clamp_min(1e-300)).max()):.3g}, first at {bad.nonzero()[0].tolist()}")


# ---- forward ---------------------------------------------------------------------------------------------------------
# input configurations: (in_a, in_b, out_dim, act, scale, extra row stride of xa, of xb)
CONFIGS = [
    (82, 0, 4, mlp.ACT_SIGMOID, 0.8, 18, 0),      # actor
    (82, 4, 1, mlp.ACT_NONE, 1.0, 0, 5),          # critic, xb a row-strided view
    (92, 4, 2, mlp.ACT_SIGMOID, 1.0, 3, 3),       # in_a + in_b = 96: the limit
    (90, 3, 3, mlp.ACT_NONE, 1.0, 7, 0),          # 93
    (5, 0, 4, mlp.ACT_NONE, 1.0, 0, 0),           # tiny input
    (3, 2, 2, mlp.ACT_SIGMOID, 0.8, 1, 2),
]


def _forward_cases():
    cases = []
    forms = ("lds", "shadow", "split2", "split4")
    for form in forms:
        for wi, hw in enumerate(NOMINAL):
            if form != "lds" and hw not in LDS_FREE:
                continue
            for ni, n in enumerate(NS):
                c = (wi + ni + forms.index(form)) % len(CONFIGS)
                cases.append((form, hw, n, c, (ni + wi) % 2 == 0))
    # partial last tiles of every tile class, with the hidden outputs (h % 4 == 0)
    for hw, n, c in (((244, 244), 17, 0), ((392, 292), 65, 1), ((120, 116), 4097, 2), ((60, 52), 63, 3), ((244, 244), 4097, 1),
                     ((60, 52), 1, 4)):
        cases.append(("lds", hw, n, c, True))
    # h % 4 != 0: the VEC=false instantiation (no hidden outputs possible)
    for hw, n, c in (((250, 250), 65, 0), ((250, 250), 4097, 1), ((390, 290), 17, 2), ((126, 126), 16, 5)):
        cases.append(("lds", hw, n, c, False))
    return cases


FORWARD_CASES = _forward_cases()


def run_forward(form, layers, xa, xb, act, scale, hid, monkeypatch):
    n = xa.shape[0]
    (W1, _), (W2, _), (W3, _) = layers
    h1o = torch.full((n, W1.shape[0]), 7.0, device=DEV) if hid else None
    h2o = torch.full((n, W2.shape[0]), 7.0, device=DEV) if hid else None
    if form != "lds":
        monkeypatch.setenv("KS_MLP_SPLIT", {"shadow": "0", "split2": "2", "split4": "4"}[form])
    out = mlp.mlp3_forward(layers, xa, xb, act=act, scale=scale, h1_out=h1o, h2_out=h2o, shadow=form != "lds")
    torch.cuda.synchronize()
    return out, h1o, h2o


@pytest.mark.parametrize("form,hw,n,cfg,hid", FORWARD_CASES, ids=[f"{f}-{h[0]}x{h[1]}-n{n}-c{c}-{'h' if hid else 'noh'}" for f, h, n, c, hid in FORWARD_CASES])
def test_forward_exact_and_bounded(form, hw, n, cfg, hid, monkeypatch):
    in_a, in_b, out_dim, act, scale, ea, eb = CONFIGS[cfg]
    in_dim = in_a + in_b
    h1, h2 = hw
    g = _gen("fwd", form, hw, n, cfg)
    # (a) exact
    L, fx, (f1, f2, f3) = exact_net(h1, h2, in_dim, out_dim, g)
    x = dyadic((n, in_dim), fx, 3, 0.7, g)
    x[::5] = 0                                       # whole zero rows: pre-activation = bias, 0 for the zero-bias units
    xa, xb = wide(x[:, :in_a], ea, g), (wide(x[:, in_a:], eb, g) if in_b else None)
    out, h1o, h2o = run_forward(form, to_dev(L), xa, xb, mlp.ACT_NONE, 1.0, hid, monkeypatch)
    (W1, b1), (W2, b2), (W3, b3) = L
    assert_exact_ok(x, W1.t(), b1, f1)
    z1 = x @ W1.t() + b1
    r1 = z1.clamp_min(0)
    assert (z1 == 0).any(), "no exactly-zero pre-activation"
    assert_exact_ok(r1, W2.t(), b2, f2)
    r2 = (r1 @ W2.t() + b2).clamp_min(0)
    assert_exact_ok(r2, W3.t(), b3, f3)
    if hid:
        check_exact(h1o, r1, "h1 exact")
        check_exact(h2o, r2, "h2 exact")
    check_exact(out, r2 @ W3.t() + b3, "out exact")
    # (b) dense
    L = dense_net(h1, h2, in_dim, out_dim, g)
    x = torch.randn(n, in_dim, generator=g, dtype=torch.float64).float().double()
    xa, xb = wide(x[:, :in_a], ea, g), (wide(x[:, in_a:], eb, g) if in_b else None)
    out, h1o, h2o = run_forward(form, to_dev(L), xa, xb, act, scale, hid, monkeypatch)
    (W1, b1), (W2, b2), (W3, b3) = L
    z1, m1 = lin(x, W1, b1)
    e1 = (in_dim + 4) * U * m1
    if hid:
        check_bound(h1o, z1.clamp_min(0), e1, "h1")
        k1 = h1o.double().cpu()
        z2, m2 = lin(k1, W2, b2)
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


# ---- backward (data gradients) ---------------------------------------------------------------------------------------
def _backward_cases():
    dxs = [None, (86, 0, 4), (86, 82, 4), (86, 85, 1), (96, 92, 4)]      # (in_dim, col0, ncol)
    dzs = [(True, True), (False, False), (True, False), (False, True)]    # (dz2_out given, dz1_out given)
    cases, i = [], 0
    for form in ("shadow", "split2", "split4"):
        for hw in LDS_FREE:
            for n in NS:
                dxc, dz = dxs[i % len(dxs)], dzs[i % len(dzs)]
                if dxc is None and dz == (False, False):
                    dxc = (86, 82, 4)
                act = dxc is not None and (i // len(dxs)) % 2 == 0
                cases.append((form, hw, n, 1 + i % 4, dz, dxc, act))
                i += 1
    return cases


BACKWARD_CASES = _backward_cases()


def run_backward(form, layers, dz3, h1, h2, want, dxc, act_out, scale, monkeypatch):
    """mlp.mlp3_backward when both or neither of dz2 / dz1 are wanted, the C ABI for one of them"""
    (W1, _), (W2, _), (W3, _) = layers
    n = dz3.shape[0]
    if want[0] == want[1]:
        monkeypatch.setenv("KS_MLP_SPLIT", {"shadow": "0", "split2": "2", "split4": "4"}[form])
        dz2, dz1, dx = mlp.mlp3_backward(layers, dz3, h1, h2, want_dz=want[0], dx_cols=None if dxc is None else dxc[1:], act_out=act_out, scale=scale)
    else:
        lib, P = ks.load_library(), ks._ptr
        dz2 = torch.full_like(h2, 7.0) if want[0] else None
        dz1 = torch.full_like(h1, 7.0) if want[1] else None
        col0, ncol = (0, 0) if dxc is None else dxc[1:]
        dx = torch.full((n, ncol), 7.0, device=DEV) if dxc is not None else None
        args = (n, W1.shape[1], W1.shape[0], W2.shape[0], W3.shape[0], P(dz3), P(W3), P(h2), P(W2), P(h1), P(dz2), P(dz1), P(W1), col0, ncol,
                P(act_out), float(scale), P(dx))
        if form == "shadow":
            rc = lib.kr_mlp3_backward_shadow(*args, _stream())
        else:
            waves = int(form[-1])
            need = (n + 15) // 16 * waves * 64
            scratch = torch.empty(need, device=DEV)
            rc = lib.kr_mlp3_backward_split(*args, P(scratch), need, waves, _stream())
        assert rc == 0
    torch.cuda.synchronize()
    return dz2, dz1, dx


@pytest.mark.parametrize("form,hw,n,out_dim,want,dxc,act", BACKWARD_CASES,
                         ids=[f"{f}-{h[0]}-n{n}-o{o}-dz{int(w[0])}{int(w[1])}-dx{d[1:] if d else None}-{'act' if a else 'lin'}"
                              for f, h, n, o, w, d, a in BACKWARD_CASES])
def test_backward_exact_and_bounded(form, hw, n, out_dim, want, dxc, act, monkeypatch):
    h1, h2 = hw
    in_dim = dxc[0] if dxc else 86
    g = _gen("bwd", form, hw, n, out_dim, want, dxc, act)
    cols = slice(dxc[1], dxc[1] + dxc[2]) if dxc else None
    # (a) exact; the sigmoid epilogue with a power-of-two scale (a / scale, 1 - a / scale, a (1 - a / scale) exact)
    d = lambda K: min(1.0, 24.0 / K)
    W1, W2, W3 = dyadic((h1, in_dim), 3, 3, d(h1), g), dyadic((h2, h1), 3, 3, d(h2), g), dyadic((out_dim, h2), 3, 3, 1.0, g)
    dz3 = dyadic((n, out_dim), 3, 3, 0.8, g)
    a1, a2 = dyadic((n, h1), 2, 3, 0.5, g, nonneg=True), dyadic((n, h2), 2, 3, 0.5, g, nonneg=True)   # stored activations, ~half zero
    scale = 0.5
    act_out = (torch.randint(1, 8, (n, dxc[2]), generator=g).double() * 2.0 ** -4) if act else None     # in (0, scale)
    dev = lambda t: None if t is None else t.float().to(DEV).contiguous()
    layers = [(dev(W1), None), (dev(W2), None), (dev(W3), None)]
    dz2, dz1, dx = run_backward(form, layers, dev(dz3), dev(a1), dev(a2), want, dxc, dev(act_out), scale, monkeypatch)
    assert_exact_ok(dz3, W3, None, 6)
    r2 = (dz3 @ W3) * (a2 > 0)
    assert_exact_ok(r2, W2, None, 9)
    r1 = (r2 @ W2) * (a1 > 0)
    if want[0]:
        check_exact(dz2, r2, "dz2 exact")
    if want[1]:
        check_exact(dz1, r1, "dz1 exact")
    if dxc:
        assert_exact_ok(r1, W1[:, cols], None, 12)
        rx = r1 @ W1[:, cols]
        if act:
            f = act_out * (1 - act_out / scale)
            assert float((rx.abs() * 2.0 ** 12 * f * 2.0 ** 8).max()) < 2.0 ** 24
            rx = rx * f
        check_exact(dx, rx, "dx exact")
    # (b) dense
    scale = 0.8
    L = dense_net(h1, h2, in_dim, out_dim, g)
    (W1, _), (W2, _), (W3, _) = L
    dz3 = torch.randn(n, out_dim, generator=g, dtype=torch.float64).float().double()
    a1 = torch.randn(n, h1, generator=g, dtype=torch.float64).float().double().clamp_min(0)
    a2 = torch.randn(n, h2, generator=g, dtype=torch.float64).float().double().clamp_min(0)
    act_out = (scale * torch.sigmoid(torch.randn(n, dxc[2], generator=g, dtype=torch.float64))).float().double() if act else None
    layers = [(dev(W1), None), (dev(W2), None), (dev(W3), None)]
    dz2, dz1, dx = run_backward(form, layers, dev(dz3), dev(a1), dev(a2), want, dxc, dev(act_out), scale, monkeypatch)
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


# ---- weight gradients ------------------------------------------------------------------------------------------------
# (n, M, Na, Nb, extra row stride of ha, of hb, rows_per_chunk)
WGRAD_CASES = [
    (1, 1, 64, 0, 0, 0, 400), (15, 4, 82, 4, 18, 3, 16), (16, 64, 256, 0, 0, 0, 100), (17, 300, 96, 0, 5, 0, 16),
    (63, 4, 256, 0, 0, 0, 400), (64, 1, 82, 4, 0, 0, 100), (65, 64, 86, 0, 2, 0, 16), (4097, 4, 256, 0, 0, 0, 400),
    (4097, 300, 82, 4, 18, 3, 400), (4097, 64, 64, 0, 0, 0, 100), (1600, 256, 256, 0, 0, 0, 400), (333, 64, 92, 4, 0, 0, 16),
    (20, 64, 96, 0, 0, 0, 8), (20, 4, 82, 4, 0, 0, 8),         # rounded to 16-row chunks: a trailing chunk past n
]


def wgrad_ref(dz, h):
    """dW = dz^T h, db = column sums of dz, and their bounds (K = n)"""
    n = dz.shape[0]
    return dz.t() @ h, dz.sum(0), (n + 4) * U * (dz.abs().t() @ h.abs()), (n + 4) * U * dz.abs().sum(0)


@pytest.mark.parametrize("n,M,Na,Nb,ea,eb,rpc", WGRAD_CASES, ids=[f"n{c[0]}-M{c[1]}-N{c[2]}+{c[3]}-rpc{c[6]}" for c in WGRAD_CASES])
def test_weight_grad_exact_and_bounded(n, M, Na, Nb, ea, eb, rpc):
    g = _gen("wgrad", n, M, Na, Nb, rpc)
    for exact in (True, False):
        if exact:
            dz, h = dyadic((n, M), 3, 3, 0.5, g), dyadic((n, Na + Nb), 2, 3, 0.5, g)
        else:
            dz = torch.randn(n, M, generator=g, dtype=torch.float64).float().double() / n
            h = torch.randn(n, Na + Nb, generator=g, dtype=torch.float64).float().double().clamp_min(0)
        ha, hb = wide(h[:, :Na], ea, g), (wide(h[:, Na:], eb, g) if Nb else None)
        dW, db = torch.full((M, Na + Nb), 7.0, device=DEV), torch.full((M,), 7.0, device=DEV)
        mlp.weight_grad(dz.float().to(DEV), ha, hb, dW, db, rows_per_chunk=rpc)
        torch.cuda.synchronize()
        rW, rb, eW, eb_ = wgrad_ref(dz, h)
        if exact:
            assert_exact_ok(dz.t(), h, None, 5)
            assert_exact_ok(dz.t(), torch.ones(n, 1, dtype=torch.float64), None, 3)
            check_exact(dW, rW, "dW exact")
            check_exact(db, rb, "db exact")
        else:
            check_bound(dW, rW, eW, "dW")
            check_bound(db, rb, eb_, "db")


@pytest.mark.parametrize("n,M,Na,Nb,chunks", [(20, 64, 64, 0, 5), (33, 4, 82, 4, 7), (17, 300, 96, 0, 2), (100, 16, 64, 0, 3)])
def test_weight_grad_abi_chunks(n, M, Na, Nb, chunks):
    """kr_weight_grad_shadow with any `chunks`, more than ceil(n / 16) included: the rows are rounded to 16-row chunks and
    chunks without rows add nothing (exact dyadic inputs: bit-equal to the fp64 sums)"""
    lib, P = ks.load_library(), ks._ptr
    g = _gen("chunks", n, M, Na, Nb, chunks)
    dz, h = dyadic((n, M), 3, 3, 0.5, g), dyadic((n, Na + Nb), 2, 3, 0.5, g)
    assert_exact_ok(dz.t(), h, None, 5)
    dzd, hd = dz.float().to(DEV), h.float().to(DEV)
    ha, hb = hd[:, :Na], (hd[:, Na:] if Nb else None)
    ws = torch.full((chunks * (M * (Na + Nb) + M),), 7.0, device=DEV)
    dW, db = torch.full((M, Na + Nb), 7.0, device=DEV), torch.full((M,), 7.0, device=DEV)
    assert lib.kr_weight_grad_shadow(n, M, Na, Nb, P(dzd), P(ha), hd.stride(0), P(hb), hd.stride(0) if Nb else 0, chunks, P(ws), P(dW), P(db), _stream()) == 0
    torch.cuda.synchronize()
    rW, rb, _, _ = wgrad_ref(dz, h)
    check_exact(dW, rW, "dW exact")
    check_exact(db, rb, "db exact")


# ---- fused actor + action selection ----------------------------------------------------------------------------------
@pytest.mark.parametrize("hw,n", [((256, 256), 16), ((400, 300), 300), ((128, 128), 17), ((64, 64), 65), ((250, 250), 33), ((120, 116), 1)])
def test_actor_select_against_fp64_and_the_separate_kernels(hw, n):
    """kr_actor_select: its actor_out within the dense bound of the fp64 actor, its actions / latches bit-equal to
    kr_mlp3_forward followed by kr_select_action on the same noise"""
    lib, P = ks.load_library(), ks._ptr
    g = _gen("select", hw, n)
    L = dense_net(hw[0], hw[1], 82, 4, g)
    Ld = to_dev(L)
    (w1, b1), (w2, b2), (w3, b3) = Ld
    x = torch.randn(n, 82, generator=g, dtype=torch.float64).float().double()
    obs = x.float().to(DEV)
    prev = torch.randn(n, 82, generator=g).to(DEV)
    prev[: n // 2, 9:16:3] = obs[: n // 2, 9:16:3]                # fingertips at rest: the grasp check fires
    has_prev = (torch.rand(n, generator=g) < 0.8).to(DEV)
    t = torch.randint(0, 30, (n,), generator=g).to(DEV)
    noise = torch.randn(n, 4, generator=g).to(DEV)
    ready = (torch.rand(n, generator=g) < 0.1).to(DEV)

    def fresh():
        return ready.clone(), torch.full((n, 4), 7.0, device=DEV), torch.full((4, n), 7.0, device=DEV), torch.zeros(n, dtype=torch.bool, device=DEV)

    r1, a1, at1, l1 = fresh()
    r2, a2, at2, l2 = fresh()
    pi = mlp.mlp3_forward(Ld, obs, act=mlp.ACT_SIGMOID, scale=0.8)
    assert lib.kr_select_action(n, P(obs), P(prev), P(has_prev), P(t), P(r1), P(pi), P(noise), 0.08, 0.8, 6, P(a1), P(at1), P(l1), _stream()) == 0
    pi2 = torch.full((n, 4), 7.0, device=DEV)
    assert lib.kr_actor_select(n, hw[0], hw[1], P(obs), P(prev), P(has_prev), P(t), P(r2), P(w1), P(b1), P(w2), P(b2), P(w3), P(b3), P(noise), 0,
                               None, 0.08, 0.8, 6, P(pi2), P(a2), P(at2), P(l2), _stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(pi, pi2) and torch.equal(a1, a2) and torch.equal(at1, at2) and torch.equal(l1, l2) and torch.equal(r1, r2)
    (W1, B1), (W2, B2), (W3, B3) = L
    z1, m1 = lin(x, W1, B1)
    e1 = (82 + 4) * U * m1
    r = z1.clamp_min(0)
    z2, _ = lin(r, W2, B2)
    e2 = e1 @ W2.abs().t() + (hw[0] + 4) * U * ((r + e1) @ W2.abs().t() + B2.abs())
    r = z2.clamp_min(0)
    z3, _ = lin(r, W3, B3)
    e3 = e2 @ W3.abs().t() + (hw[1] + 4) * U * ((r + e2) @ W3.abs().t() + B3.abs())
    a64 = 0.8 * torch.sigmoid(z3)
    check_bound(pi2, a64, sigmoid_bound(z3, e3, 0.8, a64), "actor_out")


# ---- refusals --------------------------------------------------------------------------------------------------------
def _fwd_abi(fn, n, in_a, in_b, hw, out_dim, misaligned=False, waves=None):
    """one forward call through the C ABI on sentinel-filled outputs; returns (rc, outputs unchanged)"""
    lib, P = ks.load_library(), ks._ptr
    h1, h2 = hw
    in_dim = in_a + in_b
    W = [torch.randn(h1, in_dim), torch.randn(h1), torch.randn(h2, h1), torch.randn(h2), torch.randn(out_dim, h2), torch.randn(out_dim)]
    W = [w.to(DEV) for w in W]
    xa, xb = torch.randn(n, in_a, device=DEV), (torch.randn(n, in_b, device=DEV) if in_b else None)
    out = torch.full((n, out_dim), 12345.0, device=DEV)
    h1buf = torch.full((n * h1 + 4,), 12345.0, device=DEV)
    h1o = h1buf[1:1 + n * h1] if misaligned else h1buf[:n * h1]           # 4 bytes past a 16-byte boundary
    h2o = torch.full((n, h2), 12345.0, device=DEV)
    args = (n, in_a, in_b, h1, h2, out_dim, P(xa), in_a, P(xb), in_b, *(P(w) for w in W), mlp.ACT_NONE, 1.0, P(out), P(h1o), P(h2o))
    if waves is None:
        rc = getattr(lib, fn)(*args, _stream())
    else:
        need = n * h1 + (n + 15) // 16 * waves * 64 + 64
        scratch = torch.empty(need, device=DEV)
        rc = getattr(lib, fn)(*args, P(scratch), need, waves, _stream())
    torch.cuda.synchronize()
    return rc, bool((out == 12345.0).all() and (h1buf == 12345.0).all() and (h2o == 12345.0).all())


FWD_REFUSALS = [
    # (entry point, in_a, in_b, widths, out_dim, misaligned h1_out, waves)
    ("kr_mlp3_forward", 82, 4, (200, 100), 1, False, None),           # no such tile pair
    ("kr_mlp3_forward", 93, 4, (64, 64), 1, False, None),             # in_a + in_b = 97
    ("kr_mlp3_forward", 82, 0, (64, 64), 5, False, None),             # out_dim 5
    ("kr_mlp3_forward", 82, 0, (64, 64), 4, True, None),              # misaligned h1_out
    ("kr_mlp3_forward_shadow", 82, 4, (400, 300), 1, False, None),
    ("kr_mlp3_forward_shadow", 93, 4, (64, 64), 1, False, None),
    ("kr_mlp3_forward_shadow", 82, 0, (64, 64), 5, False, None),
    ("kr_mlp3_forward_shadow", 82, 0, (64, 64), 4, True, None),
    ("kr_mlp3_forward_shadow", 82, 0, (248, 248), 4, False, None),    # h % 16 != 0 on an LDS-free form
    ("kr_mlp3_forward_split", 82, 4, (400, 300), 1, False, 2),
    ("kr_mlp3_forward_split", 93, 4, (64, 64), 1, False, 4),
    ("kr_mlp3_forward_split", 82, 0, (64, 64), 5, False, 2),
    ("kr_mlp3_forward_split", 82, 0, (64, 64), 4, True, 4),
    ("kr_mlp3_forward_split", 82, 0, (248, 248), 4, False, 2),
    ("kr_mlp3_forward_split", 82, 0, (64, 64), 4, False, 3),          # waves = 3
]


@pytest.mark.parametrize("fn,in_a,in_b,hw,out_dim,mis,waves", FWD_REFUSALS)
def test_forward_refusals_leave_the_outputs_alone(fn, in_a, in_b, hw, out_dim, mis, waves):
    rc, untouched = _fwd_abi(fn, 17, in_a, in_b, hw, out_dim, mis, waves)
    assert rc == KS_ERR_INVALID and untouched


BWD_REFUSALS = [
    # (entry point, widths, out_dim, misaligned dz1_out, (col0, ncol), waves)
    ("kr_mlp3_backward_shadow", (192, 192), 1, False, (82, 4), None),  # no such tile pair
    ("kr_mlp3_backward_shadow", (64, 64), 5, False, (82, 4), None),
    ("kr_mlp3_backward_shadow", (248, 248), 1, False, (82, 4), None),  # h % 16 != 0
    ("kr_mlp3_backward_shadow", (64, 64), 1, True, (82, 4), None),     # misaligned dz1_out
    ("kr_mlp3_backward_shadow", (64, 64), 1, False, (84, 4), None),    # dx columns past in_dim
    ("kr_mlp3_backward_split", (192, 192), 1, False, (82, 4), 2),
    ("kr_mlp3_backward_split", (64, 64), 5, False, (82, 4), 4),
    ("kr_mlp3_backward_split", (248, 248), 1, False, (82, 4), 2),
    ("kr_mlp3_backward_split", (64, 64), 1, True, (82, 4), 4),
    ("kr_mlp3_backward_split", (64, 64), 1, False, (84, 4), 2),
    ("kr_mlp3_backward_split", (64, 64), 1, False, (82, 4), 3),
]


@pytest.mark.parametrize("fn,hw,out_dim,mis,dxc,waves", BWD_REFUSALS)
def test_backward_refusals_leave_the_outputs_alone(fn, hw, out_dim, mis, dxc, waves):
    lib, P = ks.load_library(), ks._ptr
    n, in_dim, (h1, h2) = 17, 86, hw
    W1, W2, W3 = torch.randn(h1, in_dim, device=DEV), torch.randn(h2, h1, device=DEV), torch.randn(out_dim, h2, device=DEV)
    dz3, a1, a2 = torch.randn(n, out_dim, device=DEV), torch.rand(n, h1, device=DEV), torch.rand(n, h2, device=DEV)
    dz2 = torch.full((n, h2), 12345.0, device=DEV)
    dz1buf = torch.full((n * h1 + 4,), 12345.0, device=DEV)
    dz1 = dz1buf[1:1 + n * h1] if mis else dz1buf[:n * h1]
    dx = torch.full((n, 4), 12345.0, device=DEV)
    args = (n, in_dim, h1, h2, out_dim, P(dz3), P(W3), P(a2), P(W2), P(a1), P(dz2), P(dz1), P(W1), dxc[0], dxc[1], None, 1.0, P(dx))
    if waves is None:
        rc = getattr(lib, fn)(*args, _stream())
    else:
        need = (n + 15) // 16 * 4 * 64
        scratch = torch.empty(need, device=DEV)
        rc = getattr(lib, fn)(*args, P(scratch), need, waves, _stream())
    torch.cuda.synchronize()
    assert rc == KS_ERR_INVALID
    assert (dz2 == 12345.0).all() and (dz1buf == 12345.0).all() and (dx == 12345.0).all()


@pytest.mark.parametrize("case", ["chunks0", "hb_missing", "M0"])
def test_weight_grad_refusals_leave_the_outputs_alone(case):
    lib, P = ks.load_library(), ks._ptr
    n, M, Na, Nb = 20, 4, 82, 4
    dz, ha, hb = torch.randn(n, M, device=DEV), torch.randn(n, Na, device=DEV), torch.randn(n, Nb, device=DEV)
    ws = torch.full((4 * (M * (Na + Nb) + M),), 12345.0, device=DEV)
    dW, db = torch.full((M, Na + Nb), 12345.0, device=DEV), torch.full((M,), 12345.0, device=DEV)
    rc = lib.kr_weight_grad_shadow(n, 0 if case == "M0" else M, Na, Nb, P(dz), P(ha), Na, None if case == "hb_missing" else P(hb), Nb,
                                   0 if case == "chunks0" else 4, P(ws), P(dW), P(db), _stream())
    torch.cuda.synchronize()
    assert rc == KS_ERR_INVALID
    assert (ws == 12345.0).all() and (dW == 12345.0).all() and (db == 12345.0).all()


@pytest.mark.parametrize("case", ["tiles", "both_noise_sources", "no_noise_source"])
def test_actor_select_refusals_leave_the_outputs_alone(case):
    lib, P = ks.load_library(), ks._ptr
    n = 17
    h1, h2 = (200, 100) if case == "tiles" else (64, 64)
    W = [w.to(DEV) for w in (torch.randn(h1, 82), torch.randn(h1), torch.randn(h2, h1), torch.randn(h2), torch.randn(4, h2), torch.randn(4))]
    obs, prev = torch.randn(n, 82, device=DEV), torch.randn(n, 82, device=DEV)
    has_prev, t = torch.ones(n, dtype=torch.bool, device=DEV), torch.zeros(n, dtype=torch.long, device=DEV)
    ready = torch.zeros(n, dtype=torch.bool, device=DEV)
    noise = torch.randn(n, 4, device=DEV) if case != "no_noise_source" else None
    rng = torch.zeros(2, dtype=torch.long, device=DEV) if case != "tiles" else None
    if case == "no_noise_source":
        rng = None
    pi, act, act_t = torch.full((n, 4), 12345.0, device=DEV), torch.full((n, 4), 12345.0, device=DEV), torch.full((4, n), 12345.0, device=DEV)
    lifting = torch.zeros(n, dtype=torch.bool, device=DEV)
    rc = lib.kr_actor_select(n, h1, h2, P(obs), P(prev), P(has_prev), P(t), P(ready), *(P(w) for w in W), P(noise), 5, P(rng), 0.08, 0.8, 6,
                             P(pi), P(act), P(act_t), P(lifting), _stream())
    torch.cuda.synchronize()
    assert rc == KS_ERR_INVALID
    assert (pi == 12345.0).all() and (act == 12345.0).all() and (act_t == 12345.0).all() and not lifting.any() and not ready.any()
    assert rng is None or not rng.any()


SUPPORT_WIDTHS = NOMINAL + ((244, 244), (392, 292), (120, 116), (60, 52), (250, 250), (390, 290), (126, 126), (248, 248), (120, 120),
                            (200, 100), (192, 192), (256, 128))


@pytest.mark.parametrize("hw", SUPPORT_WIDTHS, ids=[f"{h[0]}x{h[1]}" for h in SUPPORT_WIDTHS])
def test_supported_says_exactly_when_the_launch_runs(hw):
    """mlp.supported(..., shadow=s) is true exactly when kr_mlp3_forward (s False) / kr_mlp3_forward_shadow (s True) accepts
    the layers (called without h1_out / h2_out, which supported() does not see)"""
    lib, P = ks.load_library(), ks._ptr
    n = 17
    for in_a, in_b, out_dim in ((82, 0, 4), (82, 4, 1), (92, 4, 1), (93, 4, 1)):
        layers = [(torch.randn(o, i, device=DEV) * 0.1, torch.zeros(o, device=DEV)) for o, i in ((hw[0], in_a + in_b), (hw[1], hw[0]), (out_dim, hw[1]))]
        (W1, b1), (W2, b2), (W3, b3) = layers
        xa, xb = torch.randn(n, in_a, device=DEV), (torch.randn(n, in_b, device=DEV) if in_b else None)
        for shadow in (False, True):
            out = torch.empty(n, out_dim, device=DEV)
            fn = lib.kr_mlp3_forward_shadow if shadow else lib.kr_mlp3_forward
            rc = fn(n, in_a, in_b, hw[0], hw[1], out_dim, P(xa), in_a, P(xb), in_b, P(W1), P(b1), P(W2), P(b2), P(W3), P(b3), mlp.ACT_NONE, 1.0,
                    P(out), None, None, _stream())
            torch.cuda.synchronize()
            assert rc in (0, KS_ERR_INVALID)
            assert mlp.supported(layers, in_a + in_b, shadow=shadow) == (rc == 0), (hw, in_a + in_b, shadow, rc)


# ---- one learner update ----------------------------------------------------------------------------------------------
class _NoStep:
    """stands in for the critic's optimizer in the reference's actor phase: the critic parameters are set from the native
    learner's flat buffer after its Adam step instead"""

    def step(self):
        pass


LEARNER_CASES = [((256, 256), "lds_free"), ((128, 128), "lds_free"), ((64, 64), "lds_free"), ((400, 300), "library_gemm"),
                 ((248, 248), "fused_lds_targets")]


@pytest.mark.parametrize("hidden,form", LEARNER_CASES, ids=[f"{h[0]}x{h[1]}-{f}" for h, f in LEARNER_CASES])
def test_learner_update_against_fp64_autograd(hidden, form):
    """learner_native's critic and actor gradients (and the three critic losses) against float64 autograd of DDPGfD's own
    phase_critic / phase_actor on the same batch and parameters: per tensor, the native error is at most 4 x that of fp32
    torch autograd on the same data, or 1e-6 of the tensor's largest entry.  The batch is masked (zero-weight rows),
    R = 37 rows is not a multiple of 16, n = 5."""
    from kinovagrasping_amd.ddpgfd import DDPGfD
    from kinovagrasping_amd.learner_native import NativeDDPGfDUpdate

    def make():
        torch.manual_seed(7)
        return DDPGfD(82, 4, 0.8, 5, hidden=hidden, device=DEV)

    p32, pn, p64 = make(), make(), make()
    for name in ("actor", "critic", "actor_target", "critic_target"):
        getattr(p64, name).double()
    p64._disc = p64._disc.double()
    nat = NativeDDPGfDUpdate(pn)
    assert nat.fused_targets and nat.shadow == (form == "lds_free") and nat.lds_free == (form == "lds_free")
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
