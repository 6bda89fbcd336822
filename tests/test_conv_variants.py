"""CPU tests of the 5x5 convolution's dispatcher (sept_conv.hip, host-only logic): every kernel instantiation of the tile
table is reached by some launch, tests/conv_cases.py launches every one of them, and a launch with no kernel is refused
with a status and text.  The answers come from sept_conv5x5_launch_variant, which calls the same choice as the launch."""
import ctypes
import os

import pytest

from tests.conv_cases import CASES, PAIRS

SCAN_W = range(1, 401)
SCAN_B = (1, 224)      # fewer than 192 workgroups at every width, and at least 192 at every width


@pytest.fixture(scope="module")
def lib():
    from sept_amd import _lib
    # the tuning variables move the choice (SEPT_CONV_OCC is read once per process): the scan is of the shipped choice
    tuning = sorted(k for k in os.environ if k.startswith("SEPT_CONV_"))
    assert not tuning, f"unset {tuning} to run the dispatcher tests"
    return _lib.lib


def _table(L):
    rows, out = [], (ctypes.c_int * 8)()
    while L.sept_conv5x5_variant_table(len(rows), out) == 0:
        rows.append(tuple(out[:8]))
    assert L.sept_conv5x5_variant_table(len(rows), out) < 0 and b"past" in L.sept_last_error()
    return rows


def _instantiated(rows):
    return {(e, f) for e, r in enumerate(rows) for f in range(6) if r[7] >> f & 1}


@pytest.fixture(scope="module")
def scan(lib):
    """(entry, form) -> set of (B, W) reaching it; and the refused (B, W, cin, cout, form) with their error text"""
    reached, refused = {}, []
    out = (ctypes.c_int * 7)()
    for cin, cout in PAIRS:
        for form in range(6):
            for B in SCAN_B:
                for W in SCAN_W:
                    st = lib.sept_conv5x5_launch_variant(B, 2, W, cin, cout, form, out)
                    if st >= 0:
                        reached.setdefault((st, form), set()).add((B, W))
                    else:
                        refused.append((B, W, cin, cout, form, st, lib.sept_last_error()))
    return reached, refused


def test_every_instantiation_is_reached(lib, scan):
    rows = _table(lib)
    inst = _instantiated(rows)
    assert len(rows) == 18 and len(inst) == 54, (len(rows), len(inst))
    reached, _ = scan
    assert set(reached) == inst, (sorted(inst - set(reached)), sorted(set(reached) - inst))
    for (e, form) in reached:   # the entry answered is one of the launch's channel pair
        cin, cout = rows[e][:2]
        assert (cin, cout) in PAIRS


def test_launch_answer_matches_the_table_entry(lib):
    rows = _table(lib)
    out = (ctypes.c_int * 7)()
    for B, H, W, cin, cout, form, entry in CASES:
        assert lib.sept_conv5x5_launch_variant(B, H, W, cin, cout, form, out) == entry
        assert rows[entry][:2] == (cin, cout) and tuple(out[:5]) == rows[entry][2:7]
        assert out[6] == 32 * rows[entry][2] * rows[entry][3]      # pixels per tile
        assert 0 < out[5] <= 160 * 1024                             # LDS bytes of the launch


def test_cases_select_their_entry_and_cover_every_instantiation(lib, scan):
    rows = _table(lib)
    out = (ctypes.c_int * 7)()
    covered = {}
    for c in CASES:
        B, H, W, cin, cout, form, entry = c
        assert lib.sept_conv5x5_launch_variant(B, H, W, cin, cout, form, out) == entry, c
        mt = out[6]
        assert (H * W) % mt != 0 and B % 8 != 0, c                 # ragged last tile, padded grid.y
        if form in (2, 3):
            assert H % 2 == 0 and W % 2 == 0, c
        covered.setdefault((entry, form), []).append((B, H, W, mt))
    reached, _ = scan
    assert set(covered) == set(reached) == _instantiated(rows)
    for (e, form), cs in covered.items():
        assert len({W for _, _, W, _ in cs}) >= 2 or len(cs) >= 2, (e, form, cs)     # two widths, or one width in both regimes
        ws = sorted(W for B, W in reached[(e, form)])
        assert min(W for _, _, W, _ in cs) == ws[0] and max(W for _, _, W, _ in cs) == ws[-1], (e, form)
        if ws[-1] >= 3:   # every tap reads the image somewhere (with H or W below 3 the outer taps only see the halo)
            assert any(H >= 3 and W >= 3 for _, H, W, _ in cs), (e, form, cs)
        if {B for B, _ in reached[(e, form)]} == set(SCAN_B):   # reached in both launch regimes: a row in each
            assert {B * -(-H * W // mt) < 192 for B, H, W, mt in cs} == {True, False}, (e, form, cs)
    for e in range(len(rows)):
        assert any(H * W < mt for (e2, _), cs in covered.items() if e2 == e for _, H, W, mt in cs), e   # a sub-tile image


def test_launches_without_a_kernel_are_refused_with_text(lib, scan):
    _, refused = scan
    assert refused
    pairs_refused = {(cin, cout, form) for _, _, cin, cout, form, _, _ in refused}
    assert (32, 64, 2) in pairs_refused and (64, 32, 4) in pairs_refused      # loader forms of the other direction
    assert any(W > 320 for _, W, cin, cout, form, _, _ in refused if (cin, cout, form) == (32, 64, 0))   # too wide for LDS
    for B, W, cin, cout, form, st, text in refused:
        assert st == -2, (B, W, cin, cout, form, st)            # SEPT_ERR_UNSUPPORTED
        assert b"no kernel" in text, (B, W, cin, cout, form, text)
    out = (ctypes.c_int * 7)()
    assert lib.sept_conv5x5_launch_variant(1, 2, 20, 48, 64, 0, out) == -2 and b"no kernel" in lib.sept_last_error()
    assert lib.sept_conv5x5_launch_variant(1, 3, 20, 64, 32, 2, out) == -2 and b"no kernel" in lib.sept_last_error()
    # argument errors
    assert lib.sept_conv5x5_launch_variant(0, 2, 20, 32, 64, 0, out) == -1
    assert lib.sept_conv5x5_launch_variant(1, 2, 20, 32, 64, 6, out) == -1
    assert lib.sept_conv5x5_launch_variant(1, 2, 20, 32, 64, 0, None) == -1
    assert lib.sept_conv5x5_variant_table(-1, out) == -1


def test_launch_answer_agrees_with_the_launch_entry_points(lib, scan):
    """The size queries of the entry points (sept_conv5x5_stats_parts / _bwsums_parts / _bnapply_parts / _act_parts) answer
    0 exactly where the launch query finds no kernel."""
    out = (ctypes.c_int * 7)()
    for cin, cout in PAIRS:
        for B in SCAN_B:
            for W in range(1, 401, 3):
                H = 2
                has = [lib.sept_conv5x5_launch_variant(B, H, W, cin, cout, f, out) >= 0 for f in range(6)]
                if cin <= cout:
                    assert (lib.sept_conv5x5_stats_parts(B, H, W, cin, cout) > 0) == has[1], (cin, cout, B, W)
                    assert (lib.sept_conv5x5_act_parts(B, H, W, cin, cout, 0) > 0) == has[4], (cin, cout, B, W)
                    assert (lib.sept_conv5x5_act_parts(B, H, W, cin, cout, 1) > 0) == has[5], (cin, cout, B, W)
                else:
                    assert (lib.sept_conv5x5_bwsums_parts(B, H, W, cin, cout) > 0) == has[1], (cin, cout, B, W)
                    assert (lib.sept_conv5x5_bnapply_parts(B, H, W, cin, cout, 0) > 0) == has[2], (cin, cout, B, W)
                    assert (lib.sept_conv5x5_bnapply_parts(B, H, W, cin, cout, 1) > 0) == has[3], (cin, cout, B, W)
