"""The frame sizes the fronts' persistent launches accept: host predicates of libaudiogan_hip.so (no GPU needed).  The
launches take any frame size that is a multiple of 8 up to the padded panel width of the state size (256 at S = 1024, 64 at
S = 128) - the reference's default frame_size = 200 among them (audiogan.py:557)."""
import ctypes

import pytest

import audiogan_amd.kernels as K
from audiogan_amd import _lib

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


# ---- the argument structs of ag_gfront_fwd / ag_gfront_bwd: what the launchers refuse, before any HIP call -----------------
# Every case here fails validation, so nothing is enqueued and no pointer is followed: the fields point at one small host
# buffer, and ws_bytes = 0 would stop a call that slipped through the rule under test at the workspace check.
_HOST = ctypes.create_string_buffer(64 + 16)
PTR = (ctypes.addressof(_HOST) + 15) & ~15
FORMS = [(0, 0), (1, 0), (0, 1), (1, 1)]        # (cell, gen): LSTM training, GRU training, LSTM generation, GRU generation
GEN_FIELDS = ('w_s', 'b_s', 'u', 's', 'first', 't_run')


def fwd_args(cell, gen, B=4, S=128, fs=64, T=2, **over):
    used = ['gates', 'w_x', 'w_hh', 'w_p', 'b_p', 'x', 'ws'] + (list(GEN_FIELDS) if gen else ['hs', 'xt'])
    used += (['b_hn'] if cell else []) + (['gh'] if cell and not gen else []) + (['cs'] if not cell and not gen else [])
    kw = dict({n: PTR for n in used}, struct_bytes=ctypes.sizeof(_lib.FrontFwdArgs), cell=cell, gen=gen, ldx=T * fs, lds=T,
              ldwx=fs, ws_bytes=0, T=T, B=B, S=S, fs=fs, n_cu=N_CU)
    kw.update(over)
    return _lib.FrontFwdArgs(**kw)


def bwd_args(cell, B=4, S=128, fs=64, T=2, **over):
    used = ['ga', 'state', 'x', 'dh_ext', 'dx_ext', 'w_hh', 'w_x', 'w_p', 'dgs', 'dxt', 'ws'] + (['gh', 'dgh'] if cell else [])
    kw = dict({n: PTR for n in used}, struct_bytes=ctypes.sizeof(_lib.FrontBwdArgs), cell=cell, ldx=T * fs, lddx=T * fs,
              ldwx=fs, ws_bytes=0, T=T, B=B, S=S, fs=fs, n_cu=N_CU)
    kw.update(over)
    return _lib.FrontBwdArgs(**kw)


def call(entry, a):
    rc = getattr(K.lib, entry)(ctypes.byref(a), None)
    return rc, K.lib.ag_last_error().decode()


@pytest.mark.parametrize('cell,gen', FORMS)
def test_a_filled_struct_reaches_the_shape_predicate(cell, gen):
    """B = 65 is past the forward's batch limit: AG_ERR_UNSUPPORTED says the struct passed the size, mode and NULL rules"""
    rc, msg = call('ag_gfront_fwd', fwd_args(cell, gen, B=65, S=1024, fs=200))
    assert rc == _lib.AG_ERR_UNSUPPORTED and 'B=65' in msg, msg


@pytest.mark.parametrize('cell', [0, 1])
def test_a_filled_backward_struct_reaches_the_shape_predicate(cell):
    rc, msg = call('ag_gfront_bwd', bwd_args(cell, n_cu=11))          # the grid is 8 + 4 workgroups
    assert rc == _lib.AG_ERR_UNSUPPORTED and '11 CUs' in msg, msg


@pytest.mark.parametrize('off', [-8, 8])
@pytest.mark.parametrize('cell,gen', FORMS)
def test_struct_size_mismatch_is_refused(cell, gen, off):
    size = ctypes.sizeof(_lib.FrontFwdArgs)
    rc, msg = call('ag_gfront_fwd', fwd_args(cell, gen, B=65, S=1024, fs=200, struct_bytes=size + off))
    assert rc == _lib.AG_ERR_ARG and 'ag_gfront_fwd' in msg and str(size + off) in msg and str(size) in msg, msg
    size = ctypes.sizeof(_lib.FrontBwdArgs)
    rc, msg = call('ag_gfront_bwd', bwd_args(cell, struct_bytes=size + off))
    assert rc == _lib.AG_ERR_ARG and 'ag_gfront_bwd' in msg and str(size + off) in msg and str(size) in msg, msg
    assert K.lib.ag_gfront_fwd(None, None) == _lib.AG_ERR_ARG and K.lib.ag_gfront_bwd(None, None) == _lib.AG_ERR_ARG


@pytest.mark.parametrize('cell,gen,field', [(0, 0, 'cs'), (1, 0, 'gh'), (0, 1, 'u'), (1, 1, 'u'), (1, 1, 'b_hn')])
def test_a_required_pointer_left_null_is_refused(cell, gen, field):
    rc, msg = call('ag_gfront_fwd', fwd_args(cell, gen, **{field: None}))
    assert rc == _lib.AG_ERR_ARG and 'ag_gfront_fwd: %s is NULL' % field in msg, msg


def test_required_backward_pointers():
    for cell, field in ((0, 'state'), (1, 'gh'), (1, 'dgh')):
        rc, msg = call('ag_gfront_bwd', bwd_args(cell, **{field: None}))
        assert rc == _lib.AG_ERR_ARG and 'ag_gfront_bwd: %s is NULL' % field in msg, msg
    for field in ('dh_ext', 'dx_ext'):          # the external gradients stay optional: the call goes on to the shape predicate
        rc, msg = call('ag_gfront_bwd', bwd_args(0, n_cu=11, **{field: None}))
        assert rc == _lib.AG_ERR_UNSUPPORTED, msg
    rc, msg = call('ag_gfront_fwd', fwd_args(0, 0, B=65, xt=None))          # and so does xt in training
    assert rc == _lib.AG_ERR_UNSUPPORTED, msg


@pytest.mark.parametrize('entry,args,field', [
    ('ag_gfront_fwd', lambda: fwd_args(1, 0, cs=PTR), 'cs'), ('ag_gfront_fwd', lambda: fwd_args(0, 1, hs=PTR), 'hs'),
    ('ag_gfront_fwd', lambda: fwd_args(1, 1, xt=PTR), 'xt'), ('ag_gfront_fwd', lambda: fwd_args(0, 0, b_hn=PTR), 'b_hn'),
    ('ag_gfront_fwd', lambda: fwd_args(0, 0, u=PTR), 'u'), ('ag_gfront_bwd', lambda: bwd_args(0, dgh=PTR), 'dgh'),
    ('ag_gfront_bwd', lambda: bwd_args(0, gh=PTR), 'gh')])
def test_a_pointer_of_another_form_is_refused(entry, args, field):
    rc, msg = call(entry, args())
    assert rc == _lib.AG_ERR_ARG and '%s: %s is not used' % (entry, field) in msg, msg


def test_bad_modes_and_empty_sequences_are_refused():
    for a, word in ((fwd_args(2, 0), 'cell'), (fwd_args(0, 2), 'gen'), (fwd_args(-1, 0), 'cell'), (fwd_args(0, 0, T=0), 'T must')):
        rc, msg = call('ag_gfront_fwd', a)
        assert rc == _lib.AG_ERR_ARG and word in msg, msg
    for a, word in ((bwd_args(2), 'cell'), (bwd_args(1, T=0), 'T must')):
        rc, msg = call('ag_gfront_bwd', a)
        assert rc == _lib.AG_ERR_ARG and word in msg, msg


@pytest.mark.parametrize('cls', [_lib.FrontFwdArgs, _lib.FrontBwdArgs])
def test_struct_layout_keeps_pointers_aligned(cls):
    """a cheap catch for an int32 inserted without its partner"""
    assert ctypes.sizeof(cls) % 8 == 0
    ptrs = [n for n, t in cls._fields_ if t is ctypes.c_void_p]
    assert len(ptrs) >= 13 and all(getattr(cls, n).offset % 8 == 0 for n in ptrs)
    assert all(getattr(cls, n).offset % 8 == 0 for n, t in cls._fields_ if t is ctypes.c_int64)
