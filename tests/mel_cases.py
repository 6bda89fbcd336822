"""The mel kernels that ship, one row per (n_fft, hop, n_mels) configuration, and the clip lengths
at which each one's edge paths run.  Shared by the GPU parity tests (tests/test_mel_gpu.py) and the
CPU check of the oracle at the same lengths (tests/test_oracle_mel.py), and the bound both hold
an fp32 result to against the float64 oracle."""
import numpy as np

from oracle import mel_oracle as mo

U32 = 2.0 ** -24   # unit roundoff of fp32

# (n_fft, hop, n_mels, kernel the plan must select, frames per tile of the launch at small batch).
# The shuffle form (sept_mel_shfl_kernel<M, hop, lanes per frame>) tiles 16 frames with sixteen lanes
# per frame and 32 with eight; the transpose form (only (400, hop 160)) launches its one-frame-group
# tile, MelCfg<10, 20, 10, 160, 1>::TILE = 24, at the batch sizes of the edge tests.
ROWS = [
    (800, 160, 80, "sept_mel_shfl_kernel<25, 160, 16>", 16),
    (800, 160, 128, "sept_mel_shfl_kernel<25, 160, 16>", 16),
    (1024, 160, 80, "sept_mel_shfl_kernel<32, 160, 16>", 16),
    (1024, 160, 128, "sept_mel_shfl_kernel<32, 160, 16>", 16),
    (1600, 160, 80, "sept_mel_shfl_kernel<50, 160, 16>", 16),
    (1600, 160, 128, "sept_mel_shfl_kernel<50, 160, 16>", 16),
    (400, 200, 128, "sept_mel_shfl_kernel<25, 200, 8>", 32),
    (400, 200, 80, "sept_mel_shfl_kernel<25, 200, 8>", 32),
    (400, 160, 128, "sept_mel_stft_kernel<10, 20, 10, 160, 2, true>", 24),
]


def row_id(row):
    return f"n{row[0]}-h{row[1]}-f{row[2]}"


def near_minimum_lengths(n_fft):
    """n_fft//2 + 1 is the reflect-pad minimum: every frame then mirrors at both clip ends."""
    return [n_fft // 2 + 1, n_fft // 2 + 2, n_fft - 1, n_fft + 1]


def partial_tile_lengths(hop, tile):
    """Ragged lengths giving T = 1 + L // hop = tile - 1, tile, tile + 1 and 2 tile + 1 frames (the
    last tile of a clip is then short by one, full, one frame long, one frame long again)."""
    return [(T - 1) * hop + (2 * T + 1) % hop for T in (tile - 1, tile, tile + 1, 2 * tile + 1)]   # odd: L % 4 != 0


def edge_lengths(n_fft, hop, tile):
    """Every edge length of a row: near-minimum, partial tiles, ~5 s in each residue class of L % 4
    (0 is the float4 interior staging path, the others are scalar), and 80159."""
    return (near_minimum_lengths(n_fft) + partial_tile_lengths(hop, tile)
            + [80000, 80001, 80002, 80003, 80159])


def fp32_resolution(audio, n_fft, F, hop):
    """(B, F, T) float64: what one fp32 rounding of a frame's spectral norm does to each mel power.

    An fp32 transform carries absolute error on every bin of the order of the unit roundoff times the
    frame's norm ||X||_2 (sum over all n_fft bins), whatever the bin's own size.  With d = U32 ||X||_2,
    a bin of power P may move by 2 sqrt(P) d + d^2, and a filter by the weighted sum of that over its
    bins.  A bin far below its frame -- a single-bin filter in a near-null, e.g. at a reflect-padded
    clip edge, where the frame is even about its centre -- cannot be resolved to a relative bound by
    any fp32 FFT (the fp32 torch oracle included); this is the absolute accuracy left to hold it to."""
    n_freq = n_fft // 2 + 1
    P = mo.mel_power_f64(audio, n_fft, n_freq, hop, fb=np.eye(n_freq))       # (B, n_freq, T)
    norm2 = 2.0 * P.sum(axis=1) - P[:, 0] - P[:, -1]                          # sum of |X_k|^2 over all n_fft bins
    d = U32 * np.sqrt(norm2)[:, None, :]
    fb = mo.melscale_fbanks_htk(n_freq, F).numpy().astype(np.float64)
    return np.einsum("kf,bkt->bft", fb, 2.0 * np.sqrt(P) * d + d * d)


def compare_fp32(got_db, audio, n_fft, F, hop, rel_power, abs_db):
    """got_db (B, F, T) dB from an fp32 path vs the float64 oracle of `audio`: every mel power within
    rel_power relative of the oracle's, or -- only where that is finer than fp32 can resolve -- within
    fp32_resolution; and within abs_db dB wherever the relative bound is the one that applies."""
    want = mo.mel_spectrogram_f64(audio, n_fft, F, hop=hop)
    got = np.asarray(got_db, dtype=np.float64)
    assert got.shape == want.shape
    pg, pw = 10 ** (got / 10), 10 ** (want / 10)
    res = fp32_resolution(audio, n_fft, F, hop)
    resolved = rel_power * pw >= res
    err = np.abs(pg - pw)
    worst = err / np.where(resolved, rel_power * pw, res)
    assert worst.max() <= 1.0, (f"mel power err {err.flat[worst.argmax()]:.3e} (power {pw.flat[worst.argmax()]:.3e}, "
                                f"fp32 resolution {res.flat[worst.argmax()]:.3e}) at {np.unravel_index(worst.argmax(), worst.shape)}")
    db = np.where(resolved, np.abs(got - want), 0.0)
    assert db.max() < abs_db, f"dB err {db.max():.3e} at {np.unravel_index(db.argmax(), db.shape)}"
    return int((~resolved).sum())
