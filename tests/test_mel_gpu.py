"""GPU parity tests of the fused STFT->mel->dB HIP kernel (through the C ABI) against the
feature oracle.  Tolerance (north-star): mel features within 1e-4 relative -- checked on
mel POWER against the float64 oracle (dB is ill-conditioned only through the power), plus
an absolute bound on dB.  Reference semantics: audio_feature_extraction.py:29-46.

Every kernel instantiation that ships is a row of tests/mel_cases.py:ROWS; each row asserts
that its plan reaches the kernel it is meant to exercise before it is compared."""
import functools
import math
import os

import numpy as np
import pytest
import torch

from oracle import mel_oracle as mo
from tests import mel_cases as mc

pytestmark = pytest.mark.gpu

REL_POWER = 1e-4
ABS_DB = 1e-3
# (n_fft, hop, F); the hop-160 rows keep the ids "n_fft-F" they had before the hop was a parameter
CASES = [pytest.param(*r[:3], id=f"{r[0]}-{r[2]}" if r[1] == 160 else f"{r[0]}-{r[2]}-h{r[1]}") for r in mc.ROWS]
ROWS = [pytest.param(r, id=mc.row_id(r)) for r in mc.ROWS]
SHFL_ROWS = [pytest.param(r, id=mc.row_id(r)) for r in mc.ROWS if r[3].startswith("sept_mel_shfl_kernel<")]
KERNEL = {r[:3]: r[3] for r in mc.ROWS}
# the transpose-form row's plan names its deep tile; launches of a few clips take its shallow one (MelCfg TILE 24)
SMALL_LAUNCH = {"sept_mel_stft_kernel<10, 20, 10, 160, 2, true>": "sept_mel_stft_kernel<10, 20, 10, 160, 1, true>"}


def _rel_power(n_fft):
    # n_fft 400 (the MFCC front end at hop 200, and hop 160) has single-bin filters: a lone fp32 FFT bin far below
    # the frame's peak carries ~1e-7 * peak absolute error, which the 1e-4 RELATIVE bound cannot absorb (the fp32
    # torch oracle itself reaches 5e-5 there, 8.3e-5 at 80 mels and hop 200).
    return REL_POWER if n_fft != 400 else 5e-4


def _fp32_check(got_db, x, n_fft, F, hop):
    """The edge tests' bound: 1e-4 relative on mel power (n_fft 400: 5e-4) and 1e-3 dB, except on the few mel
    powers finer than an fp32 transform can resolve, which are held to that resolution (mel_cases.compare_fp32)."""
    return mc.compare_fp32(got_db, np.asarray(x), n_fft, F, hop, _rel_power(n_fft), ABS_DB)


def _plan(n_fft, F, hop=160):
    from sept_amd.mel import get_mel_plan
    return get_mel_plan(n_fft, F, hop)


def _transpose_plan(monkeypatch, n_fft, F, hop):
    """A plan of the transpose form (SEPT_MEL_TRANSPOSE_FORM is read when the plan is created); the environment is
    restored before returning, so that every later plan is of the shuffle form again."""
    from sept_amd.mel import MelPlan
    with monkeypatch.context() as m:
        m.setenv("SEPT_MEL_TRANSPOSE_FORM", "1")
        plan = MelPlan(n_fft, F, hop)
    assert "SEPT_MEL_TRANSPOSE_FORM" not in os.environ
    assert plan.kernel_name.startswith("sept_mel_stft_kernel<"), plan.kernel_name
    return plan


def _hip(x, n_fft, F, layout=0, hop=160, plan=None):
    plan = plan or _plan(n_fft, F, hop)
    return plan.forward(x.cuda(), layout).cpu()


def _compare(got, want, rel_power=REL_POWER, tonal=False):
    """got, want: (B, F, T) dB.  tonal=True: pure tones / constants leave most mel bands at leakage level,
    1e-10 and more below the clip's peak -- under the fp32 noise floor of ANY fp32 FFT (the reference's
    included), where a relative bound is meaningless.  There only smallness is checked."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == want.shape
    pg, pw = 10 ** (got / 10), 10 ** (want / 10)
    sig = np.ones_like(pw, dtype=bool)
    if tonal:
        peak = pw.max(axis=(1, 2), keepdims=True)
        sig = pw > 1e-7 * peak
        assert (pg[~sig] < 1e-6 * np.broadcast_to(peak, pw.shape)[~sig]).all()
    rel = np.where(sig, np.abs(pg - pw) / np.maximum(pw, 1e-10), 0.0)
    assert rel.max() < rel_power, f"rel power err {rel.max():.3e} at {np.unravel_index(rel.argmax(), rel.shape)}"
    db = np.where(sig, np.abs(got - want), 0.0)
    assert db.max() < ABS_DB, f"dB err {db.max():.3e} at {np.unravel_index(db.argmax(), db.shape)}"


def _check(x, n_fft, F, rel_power=REL_POWER, tonal=False, hop=160, plan=None):
    got = _hip(x, n_fft, F, hop=hop, plan=plan).numpy()
    _compare(got, mo.mel_spectrogram_f64(x.numpy(), n_fft, F, hop=hop), rel_power, tonal)
    return got


def _both_layouts_vs_oracle(plan, x):
    """(B, L) clips through BFT and BTF against the f64 oracle; BTF must be BFT transposed, bit for bit."""
    n_fft, hop, F = plan.n_fft, plan.hop, plan.n_mels
    B, L = x.shape
    a = plan.forward(x.cuda(), 0).cpu()
    b = plan.forward(x.cuda(), 1).cpu()
    T = 1 + L // hop
    assert a.shape == (B, F, T) and b.shape == (B, T, F)
    assert torch.equal(a.transpose(1, 2).contiguous(), b)
    _fp32_check(a.numpy(), x.numpy(), n_fft, F, hop)
    return a


def _zero_filters(n_fft, F):
    return np.nonzero(mo.melscale_fbanks_htk(n_fft // 2 + 1, F).numpy().sum(0) == 0)[0]


# ---- one table of the kernels that ship ----
@pytest.mark.parametrize("row", ROWS)
def test_every_row_reaches_its_kernel(row):
    """A dispatch change must never silently move a row onto another kernel, and the edge lengths of a row are
    derived from the tile depth its launches of three clips use."""
    n_fft, hop, F, name, tile = row
    plan = _plan(n_fft, F, hop)
    assert plan.kernel_name == name
    for L in mc.edge_lengths(n_fft, hop, tile):
        assert plan.launch_kernel(3, L) == (SMALL_LAUNCH.get(name, name), tile)


@pytest.mark.parametrize("n_fft,hop,F", CASES)
def test_seeded_noise_vs_oracle(n_fft, hop, F):
    assert _plan(n_fft, F, hop).kernel_name == KERNEL[(n_fft, hop, F)]
    torch.manual_seed(8)
    x = torch.randn(4, 80000) * 0.1
    _check(x, n_fft, F, rel_power=_rel_power(n_fft), hop=hop)


@pytest.mark.parametrize("n_fft,F", [(800, 80), (800, 128), (1600, 80), (1024, 128)])
def test_golden_slices(n_fft, F, golden_dir):
    g = np.load(os.path.join(golden_dir, "mel_golden.npz"))
    torch.manual_seed(8)
    x = torch.randn(4, 80000) * 0.1
    got = _hip(x, n_fft, F).numpy()
    frames = list(g["frames"])
    np.testing.assert_allclose(got[:, :, frames], g[f"n{n_fft}_f{F}_slices"], rtol=1e-4, atol=1e-3)
    assert got.astype(np.float64).sum() == pytest.approx(float(g[f"n{n_fft}_f{F}_sum"]), rel=1e-5)


@pytest.mark.parametrize("n_fft,hop,F", CASES)
def test_known_answers(n_fft, hop, F):
    assert _plan(n_fft, F, hop).kernel_name == KERNEL[(n_fft, hop, F)]
    # zeros -> clamp floor -> exactly -100 dB everywhere
    assert torch.all(_hip(torch.zeros(2, 8000), n_fft, F, hop=hop) == -100.0)
    # sinusoid at a bin centre and a constant, vs the f64 oracle
    n = torch.arange(16000, dtype=torch.float64)
    x = torch.stack([torch.cos(2 * np.pi * 37 * n / n_fft), torch.ones_like(n)]).float()
    # (800, 128): filter 63 of the tone's clip sits at 1.1e-7 of the peak, just above the tonal cut, in the last
    # frames; the fp32 torch oracle is off by 9.4e-5 there (pinned by test_oracle_mel.py:
    # test_fp32_resolution_is_where_fp32_transforms_differ), the kernel by 1.05e-4
    tonal_rel = 2e-4 if (n_fft, F) == (800, 128) else _rel_power(n_fft)
    _check(x, n_fft, F, rel_power=tonal_rel, tonal=True, hop=hop)
    # impulse at a frame centre: flat unit spectrum -> mel power = filterbank column sums (all-zero filters: -100 dB)
    x = torch.zeros(1, 16000)
    x[0, hop * 40] = 1.0
    got = _hip(x, n_fft, F, hop=hop)[0, :, 40].numpy()
    colsum = mo.melscale_fbanks_htk(n_fft // 2 + 1, F).numpy().sum(0)
    live = colsum > 0
    np.testing.assert_allclose(10 ** (got[live] / 10), colsum[live], rtol=1e-4)
    assert (got[~live] == -100.0).all()


# ---- edge lengths per instantiation ----
@pytest.mark.parametrize("L", [401, 480, 799, 1599, 1600, 8000, 80000, 80159])
def test_ragged_lengths_and_edges(L):
    """Clip lengths around the reflect-pad minimum, non-multiples of the hop and of the
    tile; T = 1 + L//160 as in the reference."""
    torch.manual_seed(L)
    x = torch.randn(3, L) * 0.1
    got = _check(x, 800, 80)
    assert got.shape == (3, 80, 1 + L // 160)
    _both_layouts_vs_oracle(_plan(800, 80), x)


@pytest.mark.parametrize("row", ROWS)
def test_edge_lengths_every_kernel(row):
    """Per row: the reflect-pad minimum n_fft//2 + 1 (every frame mirrors at both clip ends) and its neighbours,
    T = TILE - 1, TILE, TILE + 1, 2 TILE + 1 frames (a partial last tile, the guarded 4-wide BFT store), ~5 s in
    each residue class of L % 4 (the float4 interior staging path, and the scalar one every later clip of the
    batch takes when L % 4 != 0), and 80159; three clips of different noise, both layouts."""
    n_fft, hop, F, _, tile = row
    plan = _plan(n_fft, F, hop)
    for L in mc.edge_lengths(n_fft, hop, tile):
        torch.manual_seed(L)
        x = torch.randn(3, L) * 0.1
        _both_layouts_vs_oracle(plan, x)


# ---- every output element written ----
@pytest.mark.parametrize("row", ROWS)
def test_every_output_element_written(row):
    """out pre-filled with NaN: an unwritten tail would survive (a fresh allocation is often zeroed)."""
    n_fft, hop, F, _, tile = row
    plan = _plan(n_fft, F, hop)
    for L in mc.near_minimum_lengths(n_fft) + mc.partial_tile_lengths(hop, tile):
        torch.manual_seed(L)
        x = (torch.randn(3, L) * 0.1).cuda()
        T = 1 + L // hop
        for layout, shape in ((0, (3, F, T)), (1, (3, T, F))):
            out = torch.full(shape, float("nan"), device="cuda")
            assert plan.forward(x, layout, out=out) is out
            nan = torch.isnan(out)
            assert not nan.any(), f"L={L} layout={layout}: unwritten {nan.nonzero()[:8].tolist()}"
            assert torch.equal(out, plan.forward(x, layout))


# ---- base-pointer alignment ----
@pytest.mark.parametrize("row", ROWS)
def test_unaligned_base_equals_aligned(row):
    """A batch 4 bytes (not 16) into a larger buffer stages every tile through the scalar path; the floats loaded
    are the same, so the result is the aligned copy's bit for bit."""
    n_fft, hop, F, _, tile = row
    plan = _plan(n_fft, F, hop)
    B = 3
    for L in (80000, mc.partial_tile_lengths(hop, tile)[-1]):
        g = torch.Generator().manual_seed(L)
        buf = (torch.randn(B * L + 4, generator=g) * 0.1).cuda()
        x = buf[1:1 + B * L].view(B, L)
        assert x.data_ptr() % 16 == 4 and x.is_contiguous()
        xa = x.clone()
        assert xa.data_ptr() % 16 == 0
        for layout in (0, 1):
            assert torch.equal(plan.forward(x, layout), plan.forward(xa, layout)), (L, layout)


# ---- persistent loop: many tiles per workgroup ----
def _batch_for_three_rounds(plan, L):
    """B with B * ceil(T / TILE) >= 3 * 256: on a grid of 256 workgroups every workgroup walks three tiles or more."""
    T = 1 + L // plan.hop
    B = 1
    while B * math.ceil(T / plan.launch_kernel(B, L)[1]) < 3 * 256:
        B += 1
    return B


@pytest.mark.parametrize("row", ROWS)
def test_persistent_loop_many_tiles_per_workgroup(row, monkeypatch):
    n_fft, hop, F, _, _ = row
    plan = _plan(n_fft, F, hop)
    L = 16000
    B = _batch_for_three_rounds(plan, L)
    g = torch.Generator().manual_seed(B)
    x = torch.randn(B, L, generator=g) * 0.1
    xd = x.cuda()
    ref = [plan.forward(xd, layout).cpu() for layout in (0, 1)]
    with monkeypatch.context() as m:
        m.setenv("SEPT_MEL_WG_PER_CU", "1")   # read on every launch: a grid of 256 workgroups
        got = [plan.forward(xd, layout).cpu() for layout in (0, 1)]
    assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])
    assert torch.equal(got[0].transpose(1, 2).contiguous(), got[1])
    idx = [0, B // 2, B - 1]
    _fp32_check(got[0][idx].numpy(), x[idx].numpy(), n_fft, F, hop)


@functools.lru_cache(maxsize=1)
def _batch256():
    g = torch.Generator().manual_seed(8)
    return (torch.randn(256, 80000, generator=g) * 0.1).clamp(-1, 1)


def _full_batch_properties(n_fft, hop, F):
    x = _batch256()
    full = _hip(x, n_fft, F, hop=hop)
    assert full.shape == (256, F, 1 + 80000 // hop) and torch.isfinite(full).all()
    idx = [0, 17, 255]
    assert torch.equal(_hip(x[idx], n_fft, F, hop=hop), full[idx])
    doubled = _hip(2 * x[:8], n_fft, F, hop=hop)
    live = torch.ones(F, dtype=torch.bool)
    live[torch.from_numpy(_zero_filters(n_fft, F))] = False              # all-zero filters stay at -100 dB
    assert torch.allclose(doubled[:, live], full[:8, live] + 10 * np.log10(4.0), atol=2e-4)
    assert (doubled[:, ~live] == -100.0).all() and (full[:, ~live] == -100.0).all()
    want = mo.mel_spectrogram_f64(x[idx].numpy(), n_fft, F, hop=hop)
    assert np.abs(full[idx].numpy() - want).max() < ABS_DB


def test_full_batch_properties():
    """BASELINE config 2 size (256 clips x 5 s): size-independent properties instead of a
    full oracle run -- batch rows are independent (a clip's features do not depend on its
    batch position), scaling the waveform by 2 adds 10 log10(4) dB, and a sample of clips
    matches the oracle."""
    _full_batch_properties(800, 160, 80)


@pytest.mark.parametrize("row", [p for p in ROWS if p.values[0][:3] != (800, 160, 80)])
def test_full_batch_properties_every_kernel(row):
    n_fft, hop, F, name, _ = row
    assert _plan(n_fft, F, hop).kernel_name == name
    _full_batch_properties(n_fft, hop, F)


# ---- both kernel forms, and both transpose-form tile depths ----
@pytest.mark.parametrize("row", SHFL_ROWS)
def test_transpose_form_vs_oracle(row, monkeypatch):
    n_fft, hop, F, name, tile = row
    plan = _transpose_plan(monkeypatch, n_fft, F, hop)
    assert _plan(n_fft, F, hop).kernel_name == name       # the cached plans are still of the shuffle form
    for L in (16000, mc.partial_tile_lengths(hop, tile)[-1], n_fft // 2 + 1):
        torch.manual_seed(L)
        _both_layouts_vs_oracle(plan, torch.randn(3, L) * 0.1)


# Per launch the transpose form takes its deep tile (two frame groups) or its shallow one (one), whichever finishes
# in fewer tile times over the persistent grid (sept_mel.hip, mel_launch_of): at 5 s clips (L = 80000) two clips
# take the shallow tile and the batch named here the deep one.  (800, 128) and (400, hop 200, 80) have one tile
# depth only: the deep tile would leave room for one workgroup per CU, so the plan launches the shallow one always.
TILE_DEPTHS = {   # (n_fft, hop, F): (B of the deep launch, kernel at B = 2, kernel at that B)
    (800, 160, 80): (16, "sept_mel_stft_kernel<20, 20, 20, 160, 1, true>", "sept_mel_stft_kernel<20, 20, 20, 160, 2, true>"),
    (800, 160, 128): (16, "sept_mel_stft_kernel<20, 20, 20, 160, 1, true>", "sept_mel_stft_kernel<20, 20, 20, 160, 1, true>"),
    (1024, 160, 80): (16, "sept_mel_stft_kernel<16, 32, 16, 160, 1, false>", "sept_mel_stft_kernel<16, 32, 16, 160, 2, false>"),
    (1024, 160, 128): (16, "sept_mel_stft_kernel<16, 32, 16, 160, 1, false>", "sept_mel_stft_kernel<16, 32, 16, 160, 2, false>"),
    (1600, 160, 80): (8, "sept_mel_stft_kernel<40, 20, 20, 160, 1, false>", "sept_mel_stft_kernel<40, 20, 20, 160, 2, false>"),
    (1600, 160, 128): (8, "sept_mel_stft_kernel<40, 20, 20, 160, 1, false>", "sept_mel_stft_kernel<40, 20, 20, 160, 2, false>"),
    (400, 200, 128): (16, "sept_mel_stft_kernel<10, 20, 10, 200, 1, true>", "sept_mel_stft_kernel<10, 20, 10, 200, 2, true>"),
    (400, 200, 80): (16, "sept_mel_stft_kernel<10, 20, 10, 200, 1, true>", "sept_mel_stft_kernel<10, 20, 10, 200, 1, true>"),
    (400, 160, 128): (16, "sept_mel_stft_kernel<10, 20, 10, 160, 1, true>", "sept_mel_stft_kernel<10, 20, 10, 160, 2, true>"),
}


@pytest.mark.parametrize("row", ROWS)
def test_transpose_form_tile_depths(row, monkeypatch):
    n_fft, hop, F, name, _ = row
    shfl = name.startswith("sept_mel_shfl_kernel<")
    plan = _transpose_plan(monkeypatch, n_fft, F, hop) if shfl else _plan(n_fft, F, hop)
    B_deep, at_two, at_deep = TILE_DEPTHS[(n_fft, hop, F)]
    L = 80000
    assert plan.launch_kernel(2, L)[0] == at_two
    assert plan.launch_kernel(B_deep, L)[0] == at_deep
    g = torch.Generator().manual_seed(n_fft + F)
    x = torch.randn(B_deep, L, generator=g) * 0.1
    _both_layouts_vs_oracle(plan, x[:2])                   # two clips: the shallow tile
    full = plan.forward(x.cuda(), 0).cpu()                                      # B_deep clips: the deep tile
    idx = [0, B_deep - 1]
    _fp32_check(full[idx].numpy(), x[idx].numpy(), n_fft, F, hop)
    assert torch.equal(plan.forward(x.cuda(), 1).cpu(), full.transpose(1, 2).contiguous())


# ---- mel counts off the multiple of 16, and all-zero filters ----
@pytest.mark.parametrize("F", [40, 23])
@pytest.mark.parametrize("n_fft,hop,name,tile", [(800, 160, "sept_mel_shfl_kernel<25, 160, 16>", 16),
                                                 (400, 200, "sept_mel_shfl_kernel<25, 200, 8>", 32)])
def test_partial_filter_tiles(n_fft, hop, name, tile, F, monkeypatch):
    """A last filter tile of F % 16 filters (stores guarded by n < F; the transpose form's (F + 1)-pitched tile)."""
    plans = [_plan(n_fft, F, hop), _transpose_plan(monkeypatch, n_fft, F, hop)]
    assert plans[0].kernel_name == name
    for plan in plans:
        for L in (16000, mc.partial_tile_lengths(hop, tile)[-1]):
            torch.manual_seed(L + F)
            _both_layouts_vs_oracle(plan, torch.randn(3, L) * 0.1)


@pytest.mark.parametrize("hop", [200, 160])
def test_all_zero_filters_are_minus_100_db(hop, monkeypatch):
    """At n_fft 400 x 128 mels four HTK filters fall between bins and are all zero: exactly -100 dB in every frame
    (the oracle gives -100.0 there too), from the shuffle form and from the transpose form."""
    zero = _zero_filters(400, 128)
    assert len(zero) == 4
    plans = [_plan(400, 128, hop)]
    if hop == 200:
        plans.append(_transpose_plan(monkeypatch, 400, 128, hop))
    torch.manual_seed(hop)
    x = torch.randn(3, 16001) * 0.1
    want = mo.mel_spectrogram_f64(x.numpy(), 400, 128, hop=hop)
    assert (want[:, zero] == -100.0).all()
    live = np.setdiff1d(np.arange(128), zero)
    for plan in plans:
        a = plan.forward(x.cuda(), 0).cpu()
        b = plan.forward(x.cuda(), 1).cpu()
        assert (a[:, zero] == -100.0).all() and (b[:, :, zero] == -100.0).all()
        assert (a[:, live] > -100.0).all()


def test_errors_and_empty():
    from sept_amd._lib import SeptError
    from sept_amd.mel import get_mel_plan
    plan = get_mel_plan(800, 80)
    with pytest.raises(SeptError):            # reflect pad needs L > n_fft/2 (torch.stft raises too)
        plan.forward(torch.zeros(1, 400).cuda())
    with pytest.raises(SeptError):            # CPU tensors are refused: no fallback
        plan.forward(torch.zeros(1, 4000))
    assert plan.forward(torch.zeros(0, 4000).cuda()).shape == (0, 80, 26)
    with pytest.raises(SeptError):
        get_mel_plan(1000, 80)


@pytest.mark.parametrize("n_fft,hop,F", CASES)
def test_time_major_layout(n_fft, hop, F):
    assert _plan(n_fft, F, hop).kernel_name == KERNEL[(n_fft, hop, F)]
    torch.manual_seed(3)
    x = torch.randn(5, 24000) * 0.1
    a = _hip(x, n_fft, F, layout=0, hop=hop)
    b = _hip(x, n_fft, F, layout=1, hop=hop)
    assert b.shape == (5, 1 + 24000 // hop, F)
    assert torch.equal(a.transpose(1, 2).contiguous(), b)


def test_drop_in_signature():
    """Reference call shape: (1, L) CPU tensor in, (1, F, T) CPU tensor out."""
    from feature_extraction.audio_feature_extraction import mel_spectrogram
    torch.manual_seed(1)
    audio = torch.randn(1, 80000) * 0.1
    out = mel_spectrogram(audio, n_fft=800, feature_len=128)
    assert out.shape == (1, 128, 501) and out.dtype == torch.float32 and not out.is_cuda
    want = mo.mel_spectrogram_torch(audio, 800, 128)
    np.testing.assert_allclose(out.numpy(), want.numpy(), rtol=1e-4, atol=1e-3)
    assert mel_spectrogram(audio).shape == (1, 128, 501)      # defaults n_fft=1024, 128 mels


# ---- MFCC front end and its helper kernels ----
def test_mfcc_with_deltas_vs_oracle():
    """mfcc(audio) of the reference (audio_feature_extraction.py:15-26): 3 x 40 coefficients, per
    clip top_db clamp, ortho DCT-II; also numpy.gradient on the device."""
    from feature_extraction.audio_feature_extraction import mfcc
    from sept_amd.mfcc import gradient1d, mfcc_batched
    torch.manual_seed(4)
    audio = torch.randn(1, 48000) * 0.1
    got = mfcc(audio)
    want = mo.mfcc_with_deltas_f64(audio.numpy())
    assert got.shape == want.shape == (1, 120, 241)
    assert np.abs(got - want).max() < 1e-3 and np.abs(got - want).mean() < 5e-5   # values are O(100)
    x = torch.randn(3, 1001)
    for h in (1.0, 2.0):
        g = gradient1d(x.cuda(), h).cpu().numpy()
        np.testing.assert_allclose(g, np.gradient(x.numpy(), h, axis=1), rtol=1e-5, atol=1e-6)
    # batched call = per-clip calls (top_db is per clip, as the reference's one-file-at-a-time loop)
    xb = torch.randn(3, 16000) * torch.tensor([[0.01], [0.1], [1.0]])
    full = mfcc_batched(xb.cuda())
    for i in range(3):
        assert torch.allclose(mfcc_batched(xb[i:i + 1].cuda()), full[i:i + 1], atol=1e-4)


@pytest.mark.parametrize("L", mc.edge_lengths(400, 200, 32))
def test_mfcc_edge_lengths_vs_oracle(L):
    """mfcc_batched against the f64 MFCC clip by clip at the hop-200 edge lengths.  The clips differ in loudness
    by 70 dB and end in silence, so the top_db floor (each clip's max - 80 dB) binds, at a different level per row."""
    from sept_amd.mfcc import mfcc_batched
    torch.manual_seed(L)
    x = torch.randn(3, L) * torch.tensor([[0.001], [0.1], [3.0]])
    x[:, L // 2:] = 0.0
    got = mfcc_batched(x.cuda()).cpu().numpy()
    assert got.shape == (3, 40, 1 + L // 200)
    for i in range(3):
        want = mo.mfcc_f64(x[i:i + 1].numpy())
        err = np.abs(got[i:i + 1] - want)
        # 1e-3 per 100 of coefficient magnitude (the bound of test_mfcc_with_deltas_vs_oracle, whose values are
        # O(100)): a frame clamped at a floor of -120 dB has coefficient 0 = 128 * -120 / sqrt(128) = -1357, a
        # 128-term fp32 sum whose rounding alone is ~1e-3
        scale = max(1.0, np.abs(want).max() / 100.0)
        assert err.max() < 1e-3 * scale and err.mean() < 5e-5, (i, err.max(), err.mean(), scale)


@pytest.mark.parametrize("where", ["first", "last"])
@pytest.mark.parametrize("n_per", [1, 255, 256, 257, 100003])
def test_topdb_clamp_vs_numpy(n_per, where):
    """sept_topdb_clamp: x = max(x, max(x) - top_db) per clip (a 256-thread tree over a strided tail), the
    maximum at the first or at the last element; max and subtraction are exact, so equality is bit for bit."""
    from sept_amd._lib import check, current_stream_ptr, lib
    g = torch.Generator().manual_seed(n_per)
    x = torch.rand(4, n_per, generator=g) * -150.0                      # dB-like, much of it below the floor
    x[:, 0 if where == "first" else -1] = torch.tensor([3.0, 20.0, 50.5, 0.25])
    want = np.maximum(x.numpy(), x.numpy().max(axis=1, keepdims=True) - np.float32(80.0))
    d = x.cuda()
    check(lib.sept_topdb_clamp(d.data_ptr(), 4, n_per, 80.0, current_stream_ptr(d.device)), "sept_topdb_clamp")
    assert np.array_equal(d.cpu().numpy(), want)


@pytest.mark.parametrize("B,L", [(1, 2), (3, 2), (3, 3), (5, 300), (2, 513)])
def test_gradient1d_edges(B, L):
    """numpy.gradient (edge order 1) at its minimum length 2, at 3 (both edges, one interior point), and over
    several rows whose length is not a multiple of 256."""
    from sept_amd.mfcc import gradient1d
    torch.manual_seed(B * 1000 + L)
    x = torch.randn(B, L)
    for h in (1.0, 2.0):
        g = gradient1d(x.cuda(), h).cpu().numpy()
        np.testing.assert_allclose(g, np.gradient(x.numpy(), h, axis=1), rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("orig,new,L", [(44100, 16000, 66150), (48000, 16000, 4801), (22050, 16000, 10000)])
def test_resample_vs_oracle(orig, new, L):
    """sept_resample_forward (polyphase sinc FIR) vs the torchaudio restatement (conv1d with stride)."""
    from feature_extraction.audio_feature_extraction import Resample
    torch.manual_seed(orig)
    x = torch.randn(2, L) * 0.3
    got = Resample(orig, new)(x.cuda()).cpu()
    want = mo.resample_torch(x, orig, new)
    assert got.shape == want.shape
    assert float((got - want).abs().max()) < 2e-5
    assert Resample(16000, 16000)(x.cuda()).data_ptr() is not None
