"""The frame sizes the fronts' persistent launches accept: host predicates of libaudiogan_hip.so (no GPU needed).  The
launches take any frame size that is a multiple of 8 up to the padded panel width of the state size (256 at S = 1024, 64 at
S = 128) - the reference's default frame_size = 200 among them (audiogan.py:557)."""
import pytest

import audiogan_amd.kernels as K

N_CU = 256

ACCEPTED = [(64, 1024, 200), (32, 1024, 200), (1, 1024, 8), (64, 1024, 104), (64, 1024, 256),
            (40, 128, 40), (64, 128, 8), (64, 128, 64)]
# not multiples of 8; wider than the panel of the state size; a state size without a persistent front
REFUSED = [(64, 1024, 100), (64, 1024, 4), (64, 1024, 264), (64, 128, 72), (64, 512, 200)]


@pytest.mark.parametrize('B,S,fs', ACCEPTED)
def test_frame_size_takes_the_persistent_launches(B, S, fs):
    assert K.lib.ag_gfront_persist_ok(B, S, fs, N_CU) == 1
    assert K.lib.ag_gfront_bwd_persist_ok(B, S, fs, N_CU) == 1


@pytest.mark.parametrize('B,S,fs', REFUSED)
def test_frame_size_keeps_the_fallback(B, S, fs):
    assert K.lib.ag_gfront_persist_ok(B, S, fs, N_CU) == 0
    assert K.lib.ag_gfront_bwd_persist_ok(B, S, fs, N_CU) == 0


def test_forward_batch_limit_is_unchanged():
    assert K.lib.ag_gfront_persist_ok(65, 1024, 200, N_CU) == 0
    assert K.lib.ag_gfront_persist_ok(64, 1024, 200, N_CU) == 1


def test_co_residency_follows_the_real_grid():
    """the backward's grid is ceil(B/32) * (S/16 + ceil(fs/16)) workgroups: 77 per clip tile at fs = 200 (80 at 256)"""
    assert K.lib.ag_gfront_bwd_persist_ok(96, 1024, 200, N_CU) == 1       # 3 * 77 = 231
    assert K.lib.ag_gfront_bwd_persist_ok(96, 1024, 256, N_CU) == 1       # 3 * 80 = 240
    assert K.lib.ag_gfront_bwd_persist_ok(128, 1024, 200, N_CU) == 0      # 4 * 77 = 308
    assert K.lib.ag_gfront_bwd_persist_ok(64, 1024, 200, 154) == 1        # 2 * 77
    assert K.lib.ag_gfront_bwd_persist_ok(64, 1024, 200, 153) == 0
    assert K.lib.ag_gfront_bwd_persist_ok(64, 1024, 208, 154) == 1        # 13 x tiles as well
    assert K.lib.ag_gfront_bwd_persist_ok(64, 1024, 216, 154) == 0        # 14 x tiles: 2 * 78
    assert K.lib.ag_gfront_persist_ok(64, 1024, 200, 255) == 0            # forward: 2 * 128 workgroups whatever fs is


def test_workspace_has_the_padded_panel_width():
    """the x exchange buffer is laid out for the padded panel (FS = 256 / 64): its size does not depend on fs"""
    ws = K.lib.ag_gfront_persist_ws_bytes
    assert ws(64, 1024, 200) == ws(64, 1024, 256)
    assert ws(1, 1024, 8) == ws(32, 1024, 256)
    assert ws(40, 128, 40) == ws(40, 128, 64)
    assert ws(64, 1024, 256) - ws(32, 1024, 256) == 2 * 32 * (1024 + 256) * 4
