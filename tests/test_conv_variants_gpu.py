"""Every kernel instantiation of the 5x5 convolution (sept_conv.hip) against a float64 reference, one test per row of
tests/conv_cases.py (each row first asserts that its launch takes the table entry it names), plus the weight-gradient
kernel (sept_conv_wgrad.hip) at the edges of its grid and of its LDS checks.

Exact runs.  Integer operands -- x in {-1, 0, 1} (about a quarter non-zero), weights in {-2 .. 2} (sparse), integer bias --
and BatchNorm parameters that are dyadic with few bits, so that every value a kernel forms before its output rounding
is exact in fp32.  Each run asserts that precondition (all terms are multiples of 2^-k and the float64 sum of their
magnitudes S stays below 2^(24-k): every partial sum is then representable).  The fp32 accumulation is then exact in ANY
order, and the bf16 output must equal the float64 reference rounded to bf16 bit for bit (torch.equal); for integer
results |ref| <= 256 that rounding is the identity.  A missed, doubled or shifted term is off by at least one unit.

Random runs.  bf16-rounded randn operands, weights scaled by 1 / sqrt(25 cin):
    |y - ref| <= 2^-8 |ref| + 2^-16 S + (1 + 2^-8) conv(e_in, |w|)
  2^-8 |ref|: the bf16 output rounding (half an ulp of an 8-bit significand).
  2^-16 S, S = conv(|x|, |w|) + |bias| in float64: the fp32 accumulation.  The products are exact; each 32x32x16 MFMA adds
    16 of them to the accumulator, so a pixel sees 25 cin / 16 <= 200 accumulations, each rounding by at most 2^-24 of a
    partial sum bounded by S: 200 * 2^-24 S < 2^-16 S.  (The naive K * 2^-24 S, K = 25 cin = 3200, is 2^-12.4 S: too loose
    to see one lost term.)
  e_in: zero for a stored input; for the loader forms the error of the staged bf16 value against its float64 restatement
    (2^-8 of it for the rounding plus 2^-20 of the magnitudes of the fp32 terms it is formed from -- a handful of
    roundings of 2^-24 each; see _lbn_input / _act64).
BatchNorm sums of the epilogues are compared with their float64 restatement from the same bf16 inputs within the fp32
summation bound (n - 1) 2^-24 sum |t| with n <= pixels per tile + partial columns.

No stray writes.  Every launch writes into the first B images of a (B + 1)-image buffer filled with bf16 NaN: the guard
image must come back bit for bit, and no NaN may remain in the first B.

References run in float64 on the CPU over images 0, B / 2 and B - 1 (the 193-image launches would cost tens of GFLOP
otherwise); the NaN guard and the statistics cover the whole batch."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from tests.conv_cases import CASES, case_id

pytestmark = pytest.mark.gpu

NAN_BF16 = 0x7FC0
U = 2.0 ** -24


def _lib():
    from sept_amd import _lib
    return _lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return 0 if t is None else t.data_ptr()


def _check(st, what):
    _lib().check(st, what)


def _sparse_int(shape, g, lo, hi, frac):
    v = torch.randint(lo, hi + 1, shape, generator=g).double()
    return v * (torch.rand(shape, generator=g) < frac).double()


def _subset(B):
    return sorted({0, B // 2, B - 1})


def _nhwc(t):
    return t.permute(0, 3, 1, 2)


def _conv64(x_nhwc, w_oihw, bias=None, dgrad=False):
    """float64 conv, pad 2.  dgrad: x holds dY of a conv with weights w (C_o, C_i, 5, 5); the result is dX = conv with the
    taps flipped and the channel roles swapped (built here, independently of sept_conv5x5_prep_weights mode 1)."""
    w = w_oihw.double()
    if dgrad:
        w = w.flip(2, 3).transpose(0, 1).contiguous()
    y = F.conv2d(_nhwc(x_nhwc.double()), w, None if bias is None else bias.double(), padding=2)
    return y.permute(0, 2, 3, 1).contiguous()


def _guarded(B, H, W, C):
    buf = torch.full((B + 1, H, W, C), float("nan"), dtype=torch.bfloat16, device="cuda")
    assert int(buf.view(torch.int16)[0, 0, 0, 0]) == NAN_BF16
    return buf


def _check_guard(buf, B):
    guard = buf[B].view(torch.int16)
    assert bool((guard == NAN_BF16).all()), "a launch wrote past the last image"
    assert not bool(torch.isnan(buf[:B].float()).any()), "a launch left pixels of the batch unwritten"


def _assert_exact(y, ref, S, k):
    """y (bf16) equals ref rounded to bf16, given that the fp32 accumulation of terms that are multiples of 2^-k is exact"""
    assert float(S.max()) * 2.0 ** k < 2.0 ** 24, "precondition: the fp32 accumulation is exact"
    want = ref.to(torch.bfloat16)
    if k == 0:
        assert float(ref.abs().max()) <= 256 and torch.equal(want.double(), ref)
    bad = y.cpu() != want
    assert not bool(bad.any()), (int(bad.sum()), bad.nonzero()[:5].tolist())


def _assert_bound(y, ref, S, conv_ein=None):
    bound = 2.0 ** -8 * ref.abs() + 2.0 ** -16 * S
    if conv_ein is not None:
        bound = bound + (1 + 2.0 ** -8) * conv_ein
    err = (y.cpu().double() - ref).abs()
    bad = err > bound
    assert not bool(bad.any()), (int(bad.sum()), float((err - bound).max()), bad.nonzero()[:5].tolist())


def _dyadic_bn(C, g, tiny):
    """BatchNorm parameters with few bits (fp32 arithmetic on them is exact): gamma in {+-1, +-0.5}, one tiny channel"""
    gamma = torch.tensor([1.0, -1.0, 0.5, -0.5])[torch.randint(0, 4, (C,), generator=g)]
    beta = torch.tensor([0.25, -0.25, 0.125, 0.5])[torch.randint(0, 4, (C,), generator=g)]
    mean = torch.tensor([0.5, -0.25, 0.0, 0.75])[torch.randint(0, 4, (C,), generator=g)]
    invstd = torch.tensor([1.0, 0.5, 2.0, 1.0])[torch.randint(0, 4, (C,), generator=g)]
    gamma[tiny], beta[tiny] = 2.0 ** -12, 0.5
    return [t.float().cuda() for t in (mean, invstd, gamma, beta)]


def _drop(B, C, g, scale):
    return ((torch.rand(B, C, generator=g) > 0.2).float() * scale).cuda()


# ---------------------------------------------------------------------------------------------------------------------
# the launches, each into a guarded output buffer
# ---------------------------------------------------------------------------------------------------------------------
def _nparts(B, H, W, mt):
    return B * ((H * W + mt - 1) // mt)


def _launch_plain(x, wt, bias, cout, stats_mt=None):
    L = _lib().lib
    B, H, W, cin = x.shape
    buf = _guarded(B, H, W, cout)
    if stats_mt is None:
        _check(L.sept_conv5x5_forward(x.data_ptr(), wt.data_ptr(), _ptr(bias), buf.data_ptr(), B, H, W, cin, cout, _stream()),
               "sept_conv5x5_forward")
        parts = None
    else:
        n = _nparts(B, H, W, stats_mt)
        assert L.sept_conv5x5_stats_parts(B, H, W, cin, cout) == n
        parts = torch.full((2 * cout, n), float("nan"), device="cuda")
        _check(L.sept_conv5x5_forward_stats(x.data_ptr(), wt.data_ptr(), _ptr(bias), buf.data_ptr(), parts.data_ptr(),
                                            B, H, W, cin, cout, _stream()), "sept_conv5x5_forward_stats")
    torch.cuda.synchronize()
    _check_guard(buf, B)
    return buf[:B], parts


def _launch_bwsums(dy, wtd, cout, ep, mt):
    """data-gradient conv with the BatchNorm backward sums epilogue: ep = ("pool", ypool, gamma, beta, drop) or
    ("ext", ext, mean, invstd, gamma, beta, drop)"""
    L = _lib().lib
    B, H, W, cin = dy.shape
    buf = _guarded(B, H, W, cout)
    n = _nparts(B, H, W, mt)
    assert L.sept_conv5x5_bwsums_parts(B, H, W, cin, cout) == n
    parts = torch.full((2 * cout, n), float("nan"), device="cuda")
    if ep[0] == "pool":
        _, yp, ga, be, dr = ep
        _check(L.sept_conv5x5_dgrad_bnsums(dy.data_ptr(), wtd.data_ptr(), buf.data_ptr(), yp.data_ptr(), ga.data_ptr(),
                                           be.data_ptr(), _ptr(dr), parts.data_ptr(), B, H, W, cin, cout, _stream()),
               "sept_conv5x5_dgrad_bnsums")
    else:
        _, ext, mu, iv, ga, be, dr = ep
        _check(L.sept_conv5x5_dgrad_bnsums_ext(dy.data_ptr(), wtd.data_ptr(), buf.data_ptr(), ext.data_ptr(), mu.data_ptr(),
                                               iv.data_ptr(), ga.data_ptr(), be.data_ptr(), _ptr(dr), parts.data_ptr(),
                                               B, H, W, cin, cout, _stream()), "sept_conv5x5_dgrad_bnsums_ext")
    torch.cuda.synchronize()
    _check_guard(buf, B)
    return buf[:B], parts


def _launch_bnapply(pre, gp, sums, bn, drop, wtd, cout, ep, mt):
    L = _lib().lib
    B, H, W, cin = pre.shape
    mean, invstd, gamma, beta = bn
    buf = _guarded(B, H, W, cout)
    parts = e_y = e_mu = e_iv = e_ga = e_be = e_dr = None
    if ep is not None:
        n = _nparts(B, H, W, mt)
        assert L.sept_conv5x5_bnapply_parts(B, H, W, cin, cout, 1) == n
        parts = torch.full((2 * cout, n), float("nan"), device="cuda")
        if ep[0] == "pool":
            _, e_y, e_ga, e_be, e_dr = ep
        else:
            _, e_y, e_mu, e_iv, e_ga, e_be, e_dr = ep
    _check(L.sept_conv5x5_dgrad_bnapply(pre.data_ptr(), gp.data_ptr(), sums.data_ptr(), mean.data_ptr(), invstd.data_ptr(),
                                        gamma.data_ptr(), beta.data_ptr(), _ptr(drop), wtd.data_ptr(), buf.data_ptr(),
                                        _ptr(e_y), _ptr(e_mu), _ptr(e_iv), _ptr(e_ga), _ptr(e_be), _ptr(e_dr), _ptr(parts),
                                        B, H, W, cin, cout, _stream()), "sept_conv5x5_dgrad_bnapply")
    torch.cuda.synchronize()
    _check_guard(buf, B)
    return buf[:B], parts


def _launch_act(ext, bn, drop, wt, bias, cout, stats_mt):
    L = _lib().lib
    B, H, W, cin = ext.shape
    mean, invstd, gamma, beta = bn
    buf = _guarded(B, H, W, cout)
    parts = None
    if stats_mt is not None:
        n = _nparts(B, H, W, stats_mt)
        assert L.sept_conv5x5_act_parts(B, H, W, cin, cout, 1) == n
        parts = torch.full((2 * cout, n), float("nan"), device="cuda")
    _check(L.sept_conv5x5_forward_act(ext.data_ptr(), mean.data_ptr(), invstd.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
                                      _ptr(drop), wt.data_ptr(), _ptr(bias), buf.data_ptr(), _ptr(parts), B, H, W, cin, cout,
                                      _stream()), "sept_conv5x5_forward_act")
    torch.cuda.synchronize()
    _check_guard(buf, B)
    return buf[:B], parts


# ---------------------------------------------------------------------------------------------------------------------
# float64 restatements of the BatchNorm expressions
# ---------------------------------------------------------------------------------------------------------------------
def _act64(ext, bn, drop):
    """dropscale * relu(ext * gamma * invstd + beta - mean * gamma * invstd) (sept_bn_relu_ext_forward) in float64, and
    the magnitude of the fp32 terms it is formed from"""
    mean, invstd, gamma, beta = [t.double().cpu() for t in bn]
    x = ext.double().cpu()
    sc = gamma * invstd
    t = x * sc + (beta - mean * sc)
    d = 1.0 if drop is None else drop.double().cpu()[:, None, None, :]
    return d * t.clamp_min(0), d * ((x * sc).abs() + beta.abs() + (mean * sc).abs())


def _windows(t):
    B, H, W, C = t.shape
    return t.view(B, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(B, H // 2, W // 2, 4, C)


def _unwindows(t4):
    B, Hh, Wh, _, C = t4.shape
    return t4.view(B, Hh, Wh, 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(B, 2 * Hh, 2 * Wh, C)


def _pool_block64(x1, bn, drop):
    """BatchNorm + ReLU + MaxPool 2x2 of x1 in float64: (active [B,Hp,Wp,C], xhat at the window's first maximum)"""
    mean, invstd, gamma, beta = [t.double().cpu() for t in bn]
    x4 = _windows(x1.double().cpu())
    r = ((x4 - mean) * invstd * gamma + beta).clamp_min(0)
    best, arg = r.max(3)          # first maximum in scan order
    active = best > 0
    if drop is not None:
        active = active & (drop.double().cpu()[:, None, None, :] > 0)
    xh = (torch.gather(x4, 3, arg.unsqueeze(3)).squeeze(3) - mean) * invstd
    return active, xh


def _lbn_input(pre, gp, sums, bn, drop):
    """the gradient of the block's pre-activations the LBN loader stages (sept_bn_bwd_apply_kernel's expression) in float64:
    d = sc (ge - m1 - xhat m2) with ge the pooled gradient (times dropscale) at the window's first maximum where the ReLU is
    active; and e_in, the bound on |staged - d|: half a bf16 ulp of d + 2^-20 of the fp32 terms (sc ge, kb = -sc m1 - kc
    mean, kc x with kc = -sc invstd m2).  Where the ReLU decision could differ from the fp32 one (a channel whose
    pre-activation scale is tiny ties windows that float64 tells apart), e_in also covers |sc ge| at every window position."""
    B, H, W, C = pre.shape
    mean, invstd, gamma, beta = [t.double().cpu() for t in bn]
    x = pre.double().cpu()
    n = float(B * H * W)
    s = sums.double().cpu()
    m1, m2 = s[:C] / n, s[C:] / n
    sc = gamma * invstd
    x4 = _windows(x)
    r = (x4 * sc + (beta - mean * sc)).clamp_min(0)
    best, arg = r.max(3)
    g = gp.double().cpu() * (1.0 if drop is None else drop.double().cpu()[:, None, None, :])
    ge = torch.where(best > 0, g, torch.zeros_like(g))
    ge4 = torch.zeros_like(x4).scatter_(3, arg.unsqueeze(3), ge.unsqueeze(3))
    kc = -sc * invstd * m2
    d = _unwindows(ge4) * sc + (-sc * m1 - kc * mean) + kc * x
    T = _unwindows(ge4).abs() * sc.abs() + (sc * m1).abs() + 2 * (kc * mean).abs() + (kc * x).abs()
    e_in = 2.0 ** -8 * d.abs() + 2.0 ** -20 * T
    tiny = gamma.abs() < 1e-3
    e_in = e_in + tiny * _unwindows(ge.abs().unsqueeze(3).expand(-1, -1, -1, 4, -1)) * sc.abs()
    return d, e_in


def _sums_bound(terms, mt, nparts):
    return (mt + nparts + 64) * U * terms.abs().sum((0, 1, 2))


def _check_bwsums(parts, y, ep, mt, exclude_tiny):
    """the epilogue's (sum g, sum g xhat), finished by sept_bn_bwd_sums_from_partials, against their float64 restatement
    from the kernel's own output and the same bf16 inputs (sept_conv5x5_dgrad_bnsums / _ext's expressions)"""
    L = _lib().lib
    C, n = parts.shape[0] // 2, parts.shape[1]
    sums = torch.empty(2 * C, device="cuda")
    _check(L.sept_bn_bwd_sums_from_partials(parts.data_ptr(), n, C, sums.data_ptr(), None, None, _stream()),
           "sept_bn_bwd_sums_from_partials")
    torch.cuda.synchronize()
    yv = y.double().cpu()
    if ep[0] == "pool":
        _, yp, ga, be, dr = ep
        d = dr.double().cpu()[:, None, None, :]
        rd = torch.where(d > 0, 1.0 / d, torch.zeros_like(d))
        yy = yp.double().cpu() * rd
        ge = torch.where(yy > 0, yv * d, torch.zeros_like(yv))
        t2 = ge * (yy - be.double().cpu()) / ga.double().cpu()
        m2 = ge.abs() * (yy.abs() + be.double().cpu().abs()) / ga.double().cpu().abs()   # (the fp32 terms xhat is formed from)
    else:
        _, ext, mu, iv, ga, be, dr = ep
        e = ext.double().cpu()
        mu, iv, ga, be = [t.double().cpu() for t in (mu, iv, ga, be)]
        d = dr.double().cpu()[:, None, None, :]
        active = e * (ga * iv) + (be - mu * ga * iv) > 0
        ge = torch.where(active, yv * d, torch.zeros_like(yv))
        t2 = ge * ((e - mu) * iv)
        m2 = ge.abs() * (e.abs() + mu.abs()) * iv
    got = sums.double().cpu()
    for k, (t, m) in enumerate(((ge, ge), (t2, m2))):
        want, tol = t.sum((0, 1, 2)), _sums_bound(m, mt, n)
        ok = (got[k * C:(k + 1) * C] - want).abs() <= tol
        if exclude_tiny is not None:
            ok = ok | exclude_tiny
        assert bool(ok.all()), (k, (got[k * C:(k + 1) * C] - want).abs().max(), tol.max())
    return sums


def _check_stats(parts, y, mt):
    """statistics partials of the output: the column sums against float64 sums of the output, and mean / invstd of
    sept_bn_stats_from_partials against float64 (biased variance, eps 1e-5)"""
    L = _lib().lib
    B, H, W, C = y.shape
    yv = y.double().cpu().reshape(-1, C)
    p = parts.double().cpu()
    assert bool(torch.isfinite(p).all())
    for k, t in enumerate((yv, yv * yv)):
        assert bool(((p[k * C:(k + 1) * C].sum(1) - t.sum(0)).abs() <= (mt + 64) * U * t.abs().sum(0)).all()), k
    mean, invstd = torch.empty(C, device="cuda"), torch.empty(C, device="cuda")
    _check(L.sept_bn_stats_from_partials(parts.data_ptr(), parts.shape[1], B * H * W, C, mean.data_ptr(), invstd.data_ptr(),
                                         None, None, None, 0.1, 1e-5, _stream()), "sept_bn_stats_from_partials")
    m64, v64 = yv.mean(0), yv.var(0, unbiased=False)
    assert torch.allclose(mean.double().cpu(), m64, rtol=1e-6, atol=1e-6 * float(yv.abs().mean()))
    assert torch.allclose(invstd.double().cpu(), (v64 + 1e-5).rsqrt(), rtol=1e-5)
    return mean, invstd


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=[case_id(c) for c in CASES])
def test_conv_variant_against_float64(case):
    from sept_amd import ops
    B, H, W, cin, cout, form, entry = case
    L = _lib().lib
    out = (ctypes.c_int * 7)()
    assert L.sept_conv5x5_launch_variant(B, H, W, cin, cout, form, out) == entry
    mt = out[6]
    dgrad = cin > cout
    g = torch.Generator().manual_seed(hash(case) & 0xFFFFFFF)
    idx = _subset(B)
    tiny = 3
    # ---- weights: (C_o, C_i, 5, 5) of the conv whose forward (cin <= cout) or data gradient (cin > cout) is launched ----
    wshape = (cin, cout, 5, 5) if dgrad else (cout, cin, 5, 5)
    w_int = _sparse_int(wshape, g, -2, 2, 0.3)
    wt_int = ops.conv5x5_prep_weights(w_int.float().cuda(), 1 if dgrad else 0)
    w_rnd = (torch.randn(wshape, generator=g) / (25 * cin) ** 0.5).bfloat16().double()
    wt_rnd = ops.conv5x5_prep_weights(w_rnd.float().cuda(), 1 if dgrad else 0)
    wabs_int, wabs_rnd = w_int.abs(), w_rnd.abs()
    bias_int = None if dgrad else torch.randint(-3, 4, (cout,), generator=g).double()
    bias_rnd = None if dgrad else (0.1 * torch.randn(cout, generator=g)).double()

    def ref(inp, w, bias):
        return _conv64(inp[idx], w, bias, dgrad)

    def S(inp, wabs, bias):
        return _conv64(inp[idx].abs(), wabs, None if bias is None else bias.abs(), dgrad)

    if form in (0, 1):
        # ---- exact run ----
        x = _sparse_int((B, H, W, cin), g, -1, 1, 0.25)
        xd = x.bfloat16().cuda()
        bd = None if bias_int is None else bias_int.float().cuda()
        if form == 0 or not dgrad:
            y, parts = _launch_plain(xd, wt_int, bd, cout, mt if form == 1 else None)
            _assert_exact(y[idx], ref(x, w_int, bias_int), S(x, wabs_int, bias_int), 0)
            if form == 1:
                assert torch.equal(y, ops.conv5x5(xd, wt_int, bd))       # the statistics form computes the plain form's bits
                _check_stats(parts, y, mt)
        else:
            eps = [("pool",)] + ([("ext",)] if cout <= 32 else [])
            for kind, in eps:
                plain = ops.conv5x5(xd, wt_int)
                if kind == "pool":
                    # the block in front: pre-activations x1 (B, 2H, 2W, cout) with dyadic BatchNorm parameters, so that its
                    # pooled output -- the epilogue's input -- is exact in bf16 except in the tiny-gamma channel
                    x1 = _sparse_int((B, 2 * H, 2 * W, cout), g, -3, 3, 0.9).bfloat16().cuda()
                    bn = _dyadic_bn(cout, g, tiny)
                    dr = _drop(B, cout, g, 2.0)
                    yp = ops.bn_relu_pool_forward(x1, *bn, dr, 2)
                    ep = ("pool", yp, bn[2], bn[3], dr)
                else:
                    ext = _sparse_int((B, H, W, cout), g, -3, 3, 0.9).bfloat16().cuda()
                    bn = _dyadic_bn(cout, g, tiny)
                    dr = _drop(B, cout, g, 2.0)
                    ep = ("ext", ext, *bn, dr)
                y, parts = _launch_bwsums(xd, wt_int, cout, ep, mt)
                want = ref(x, w_int, None)
                if kind == "ext":   # the output is stored masked: zero where the block's ReLU is inactive
                    mu, iv, ga, be = [t.double().cpu() for t in bn]
                    e = ext.double().cpu()[idx]
                    want = torch.where(e * (ga * iv) + (be - mu * ga * iv) > 0, want, torch.zeros_like(want))
                    ops.bn_backward_sums_ext(plain, ext, *bn, dr)              # the unfused pair masks `plain` in place
                _assert_exact(y[idx], want, S(x, wabs_int, None), 0)
                assert torch.equal(y, plain)
                sums = _check_bwsums(parts, y, ep, mt, (bn[2].abs() < 1e-3).cpu().double() > 0 if kind == "pool" else None)
                if kind == "pool":
                    # finished as the step does: the tiny-gamma channel is recomputed from the windows of x1
                    _, dgam, dbet = ops.bn_relu_pool_backward_presummed(y, x1, *bn, dr, (parts, parts.shape[1]), 2)
                    active, xh = _pool_block64(x1, bn, dr)
                    gd = torch.where(active, y.double().cpu() * dr.double().cpu()[:, None, None, :], torch.zeros(()).double())
                    for got_, t in ((dbet, gd), (dgam, gd * xh)):
                        tol = _sums_bound(t, mt, parts.shape[1])
                        assert bool(((got_.double().cpu() - t.sum((0, 1, 2))).abs() <= tol).all()), (kind, got_, t.sum((0, 1, 2)))
                else:
                    assert bool(torch.isfinite(sums).all())
        # ---- random run ----
        x = torch.randn(B, H, W, cin, generator=g).bfloat16().double()
        xd = x.bfloat16().cuda()
        bd = None if bias_rnd is None else bias_rnd.float().cuda()
        if form == 0 or not dgrad:
            y, _ = _launch_plain(xd, wt_rnd, bd, cout, mt if form == 1 else None)
        else:
            e_bn = _dyadic_bn(cout, g, tiny)
            yp = torch.relu(torch.randn(B, H, W, cout, generator=g)).bfloat16().cuda()
            y, _ = _launch_bwsums(xd, wt_rnd, cout, ("pool", yp, e_bn[2], e_bn[3], _drop(B, cout, g, 1.25)), mt)
        _assert_bound(y[idx], ref(x, w_rnd, None if bd is None else bd.double().cpu()),
                      S(x, wabs_rnd, None if bd is None else bd.double().cpu()))
    elif form in (4, 5):
        # ---- exact run: dyadic BatchNorm of the pool-first block; the staged activation is bf16(exact value) ----
        ext = _sparse_int((B, H, W, cin), g, -2, 2, 0.6)
        extd = ext.bfloat16().cuda()
        bn = _dyadic_bn(cin, g, tiny)
        dr = _drop(B, cin, g, 2.0)
        bd = bias_int.float().cuda()
        y, parts = _launch_act(extd, bn, dr, wt_int, bd, cout, mt if form == 5 else None)
        act, _ = _act64(extd, bn, dr)
        act_b = act.to(torch.bfloat16).double()                    # (exact fp32 value, one rounding: the tile's bf16)
        _assert_exact(y[idx], ref(act_b, w_int, bias_int), S(act_b, wabs_int, bias_int), 12)
        stored = ops.bn_relu_ext_forward(extd, None, *bn, dr)
        assert torch.equal(stored.cpu().double(), act_b)
        assert torch.equal(y, ops.conv5x5(stored, wt_int, bd))       # the unfused pair, bit for bit
        if form == 5:
            mean, invstd = _check_stats(parts, y, mt)
            want = ops.conv5x5_forward_stats(stored, wt_int, bd)
            assert want is not None and torch.equal(want[0], y) and torch.equal(want[1], mean) and torch.equal(want[2], invstd)
        # ---- random run ----
        extd = (torch.randn(B, H, W, cin, generator=g) * 1.5).bfloat16().cuda()
        mean, invstd = (0.2 * torch.randn(cin, generator=g)).cuda(), (0.5 + torch.rand(cin, generator=g)).cuda()
        gamma, beta = (1 + 0.3 * torch.randn(cin, generator=g)), (0.5 + 0.2 * torch.randn(cin, generator=g))
        gamma[tiny], gamma[5] = 1e-4, -0.8
        bn = (mean, invstd, gamma.cuda(), beta.cuda())
        dr = _drop(B, cin, g, 1.25)
        bd = bias_rnd.float().cuda()
        y, _ = _launch_act(extd, bn, dr, wt_rnd, bd, cout, None)
        act, T = _act64(extd, bn, dr)
        e_in = 2.0 ** -8 * act + 2.0 ** -20 * T
        _assert_bound(y[idx], ref(act, w_rnd, bias_rnd.float().double()), S(act, wabs_rnd, bias_rnd.float().double()),
                      _conv64(e_in[idx], wabs_rnd, None, False))
        assert torch.equal(y, ops.conv5x5(ops.bn_relu_ext_forward(extd, None, *bn, dr), wt_rnd, bd))
    else:
        # ---- LBN: random run against the float64 apply pass + conv; the unfused pair within the existing bounds ----
        pre = (torch.randn(B, H, W, cin, generator=g) * 1.3).bfloat16().cuda()
        gp = torch.randn(B, H // 2, W // 2, cin, generator=g).bfloat16().cuda()
        bn = _dyadic_bn(cin, g, tiny)     # (dyadic: the fp32 ReLU / arg-max decisions are the float64 ones)
        dr = _drop(B, cin, g, 1.25)
        sums, _, _ = ops.bn_backward_sums(gp, pre, *bn, dr, 2, need_param_grads=False)
        dpre, _, _ = ops.bn_relu_pool_backward(gp, pre, *bn, dr, 2, need_param_grads=False)
        d, e_in = _lbn_input(pre, gp, sums, bn, dr)
        eps = [None] if form == 2 else [("pool",)] + ([("ext",)] if cout <= 32 else [])
        for epk in eps:
            ep = want_sums = None
            plain = ops.conv5x5(dpre, wt_rnd)
            if epk is not None and epk[0] == "pool":
                e_bn = [t.cuda() for t in ((0.1 * torch.randn(cout, generator=g)), (0.5 + torch.rand(cout, generator=g)),
                                           (1 + 0.3 * torch.randn(cout, generator=g)), (0.2 * torch.randn(cout, generator=g)))]
                e_bn[2][1] = 2e-5
                e_dr = _drop(B, cout, g, 1.25)
                yp = torch.relu(torch.randn(B, H, W, cout, generator=g)).bfloat16().cuda()
                ep = ("pool", yp, e_bn[2], e_bn[3], e_dr)
                want, want_sums = ops.conv5x5_dgrad_bnsums(dpre, wt_rnd, yp, e_bn[2], e_bn[3], e_dr)
            elif epk is not None:
                e_bn = _dyadic_bn(cout, g, 1)
                e_dr = _drop(B, cout, g, 2.0)
                ext = (torch.randn(B, H, W, cout, generator=g) * 1.5).bfloat16().cuda()
                ep = ("ext", ext, *e_bn, e_dr)
                want, want_sums = ops.conv5x5_dgrad_bnsums_ext(dpre, wt_rnd, ext, *e_bn, e_dr)
            else:
                want = plain
            y, parts = _launch_bnapply(pre, gp, sums, bn, dr, wt_rnd, cout, ep, mt)
            r = ref(d, w_rnd, None)
            if ep is not None and ep[0] == "ext":
                mu, iv, ga, be = [t.double().cpu() for t in e_bn]
                e = ext.double().cpu()[idx]
                r = torch.where(e * (ga * iv) + (be - mu * ga * iv) > 0, r, torch.zeros_like(r))
            _assert_bound(y[idx], r, S(d, wabs_rnd, None), _conv64(e_in[idx], wabs_rnd, None, True))
            # the unfused pair (apply pass, then the conv on the stored gradient): single bf16 roundings of the staged
            # gradient may differ (the loader folds sc (ge - m1 - xhat m2) into sc ge + kb + kc x)
            w32, g32 = want.float(), y.float()
            assert float((g32 - w32).norm() / w32.norm()) < 3e-3
            assert float((g32 - w32).abs().max()) < 2e-2 * float(w32.abs().max())
            if ep is not None:
                _check_bwsums(parts, y, ep, mt, (e_bn[2].abs() < 1e-3).cpu() if ep[0] == "pool" else None)
                if ep[0] == "pool":
                    a = parts.sum(1)
                    b = want_sums[0][:2 * cout * want_sums[1]].view(2 * cout, -1).sum(1)
                    assert torch.allclose(a, b, rtol=5e-3, atol=5e-3 * float(b.abs().max()))


# ---------------------------------------------------------------------------------------------------------------------
# weight gradient: sept_conv5x5_backward_weight, instantiations <32, 64, 2, 1>, <64, 128, 1, 2>, <128, 128, 1, 2>
# ---------------------------------------------------------------------------------------------------------------------
# Widest W its LDS checks accept (sept_conv_wgrad.hip, launch_wgrad): 128-pixel tiles; nr_max = (126 + W) / W + 5 staged
# rows of W + 4 pixels at PSX = wg_ps(32 NBZ) bytes and the 128 dY pixels at PSY = wg_ps(32 MBZ) bytes, double-buffered,
# within 160 KiB.  32 -> 64 (PSX 64, PSY 192): W = 145 takes 2 (6 * 149 * 64 + 128 * 192) = 163584 B, W = 146 164352 B.
# 64 -> 128 and 128 -> 128 (PSX 192, PSY 64): W = 44 takes 2 (8 * 48 * 192 + 128 * 64) = 163840 B, W = 45 166912 B; W = 1
# and 2 stage 132 and 69 rows and do not fit either (narrower images are refused too).
WGRAD_WIDEST = {(32, 64): 145, (64, 128): 44, (128, 128): 44}
WGRAD_REFUSED_NARROW = {(32, 64): (), (64, 128): (1, 2), (128, 128): (1, 2)}
WGRAD_G = {(32, 64): 256, (64, 128): 64, (128, 128): 32}    # workgroups of the grid: 256 / Z, Z = channel-block slices


def _wgrad_cases():
    cases = []
    for (cin, cout), G in WGRAD_G.items():
        Wmax = WGRAD_WIDEST[(cin, cout)]
        narrow = [w for w in (1, 2, 5) if w not in WGRAD_REFUSED_NARROW[(cin, cout)]] + [3]
        cases.append((2, 9, 13, cin, cout))                        # 2 tiles: fewer than G
        cases += [(3, 11, W, cin, cout) for W in sorted(set(narrow))]
        cases.append((2, 3, Wmax, cin, cout))                      # widest accepted
    cases += [(3, 100, 110, 32, 64), (7, 50, 25, 64, 128), (5, 21, 44, 128, 128)]   # 258, 70, 40 tiles: G does not divide
    return cases


@pytest.mark.parametrize("B,H,W,cin,cout", _wgrad_cases())
def test_conv_weight_gradient_exact(B, H, W, cin, cout):
    from sept_amd import ops
    tiles = B * -(-H * W // 128)
    G = WGRAD_G[(cin, cout)]
    if (B, H, W) in ((3, 100, 110), (7, 50, 25), (5, 21, 44)):
        assert tiles > G and tiles % G != 0
    g = torch.Generator().manual_seed(B * 7919 + H * 31 + W + cin)
    x = _sparse_int((B, H, W, cin), g, -1, 1, 0.3)
    dy = _sparse_int((B, H, W, cout), g, -1, 1, 0.3)
    dw = ops.conv5x5_backward_weight(x.bfloat16().cuda(), dy.bfloat16().cuda()).cpu().double()
    want = torch.nn.grad.conv2d_weight(_nhwc(x), (cout, cin, 5, 5), _nhwc(dy), padding=2)
    assert float(want.abs().max()) < 2 ** 24
    assert torch.equal(dw, want), (dw - want).abs().max()


@pytest.mark.parametrize("cin,cout", list(WGRAD_WIDEST))
def test_conv_weight_gradient_refuses_what_its_lds_cannot_hold(cin, cout):
    L = _lib().lib
    ws = torch.empty(L.sept_conv5x5_wgrad_workspace_floats(cin, cout), device="cuda")
    dw = torch.empty(cout, cin, 5, 5, device="cuda")
    for W in (WGRAD_WIDEST[(cin, cout)] + 1,) + WGRAD_REFUSED_NARROW[(cin, cout)]:
        x = torch.zeros(1, 2, W, cin, dtype=torch.bfloat16, device="cuda")
        dy = torch.zeros(1, 2, W, cout, dtype=torch.bfloat16, device="cuda")
        st = L.sept_conv5x5_backward_weight(x.data_ptr(), dy.data_ptr(), ws.data_ptr(), dw.data_ptr(), 1, 2, W, cin, cout,
                                            _stream())
        assert st == -2 and b"sept_conv5x5_backward_weight" in L.sept_last_error(), (W, st)
