"""The stacked front's backward through time in one launch (ag_gfront_stack_bwd), everything that needs no GPU: the shape
predicate of libaudiogan_hip.so, what the launcher refuses before any HIP call, the bindings, the switches of
K.gfront_stack_bwd_ok, the host routing of recurrent.GFrontFn.backward on a torch model of the launch's contract
(tests/stacked_front_bwd_cases.py), and the checkers of the GPU test shown to reject subtly wrong launches.  The real launch:
tests/test_gpu_front_stack_bwd.py (-m gpu)."""
import collections
import ctypes

import pytest
import torch

import audiogan_amd.kernels as K
from audiogan_amd import _lib
from tests import kernel_model
from tests import recurrent_cases as RC
from tests import stacked_front_bwd_cases as BC
from tests import stacked_front_cases as SC

N_CU = BC.N_CU


# ---- the shape predicate ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', BC.BWD_CASES, ids=SC.case_name)
def test_every_case_takes_the_one_launch_backward(case):
    assert K.lib.ag_gfront_stack_bwd_ok(case['B'], case['S'], case['fs'], case['nl'], N_CU) == 1


@pytest.mark.parametrize('nl,S,fs,B', BC.BWD_REFUSED)
def test_shapes_outside_the_rule_keep_the_per_frame_chain(nl, S, fs, B):
    assert K.lib.ag_gfront_stack_bwd_ok(B, S, fs, nl, N_CU) == 0


def test_the_predicates_table():
    """ceil(B/32) * (nl * S/16 + ceil(fs/16)) workgroups on min(n_cu, 256) CUs"""
    ok = K.lib.ag_gfront_stack_bwd_ok
    assert ok(32, 1024, 200, 2, 256) == 1 and ok(32, 1024, 200, 2, 141) == 1 and ok(32, 1024, 200, 2, 140) == 0      # 128 + 13
    assert ok(32, 1024, 200, 3, 256) == 1 and ok(32, 1024, 200, 3, 205) == 1 and ok(32, 1024, 200, 3, 204) == 0      # 192 + 13
    assert ok(64, 128, 64, 8, 256) == 1 and ok(64, 128, 64, 8, 136) == 1 and ok(64, 128, 64, 8, 135) == 0            # 2 * (64 + 4)
    assert ok(33, 1024, 200, 2, 256) == 0 and ok(33, 1024, 200, 2, 512) == 0          # 282: at most 256, whatever the chip has
    assert ok(32, 1024, 200, 4, 304) == 0                                              # 269
    assert ok(32, 1024, 208, 2, 141) == 1 and ok(32, 1024, 216, 2, 141) == 0          # 13 / 14 x tiles
    assert ok(0, 128, 64, 2, 256) == 0 and ok(-1, 128, 64, 2, 256) == 0
    for B in (1, 32, 64):
        assert ok(B, 128, 64, 1, 256) == 0 and ok(B, 128, 64, 0, 256) == 0            # one layer stays on ag_gfront_bwd
        for nl in range(2, 9):
            for fs in (8, 24, 40, 64):
                assert ok(B, 128, fs, nl, 256) == 1, (B, nl, fs)                      # every stacked front at S = 128
    assert K.lib.ag_gfront_stack_bwd_ws_bytes(32, 1024, 200, 2) == 256 + 8192           # dgs / dxt are the exchange buffers
    assert K.lib.ag_gfront_stack_bwd_ws_bytes(64, 128, 64, 8) == 256 + 8192


# ---- the argument struct: what the launcher refuses, before any HIP call ------------------------------------------------
# Every case here fails validation, so nothing is enqueued and no pointer is followed: the fields point at one small host
# buffer, and ws_bytes = 0 would stop a call that slipped through the rule under test at the workspace check.
_HOST = ctypes.create_string_buffer(64 + 16)
PTR = (ctypes.addressof(_HOST) + 15) & ~15
SIZE = ctypes.sizeof(_lib.FrontStackBwdArgs)
TABLES = ('ga', 'cs', 'w_hh', 'w_in', 'dgs')


def bwd_args(nl=2, B=4, S=128, fs=64, T=2, tables=None, **over):
    kw = dict({n: PTR for n in ('w_p', 'x', 'dh_ext', 'dx_ext', 'dxt', 'ws')}, struct_bytes=SIZE, nl=nl, ldx=T * fs, lddx=T * fs,
              ldwx=fs, ws_bytes=0, T=T, B=B, S=S, fs=fs, n_cu=N_CU)
    kw.update(over)
    a = _lib.FrontStackBwdArgs(**kw)
    for name in TABLES:
        for i in range(max(min(nl, 8), 0)):
            getattr(a, name)[i] = PTR
    for (name, i), v in (tables or {}).items():
        getattr(a, name)[i] = v
    return a


def call(a):
    rc = K.lib.ag_gfront_stack_bwd(ctypes.byref(a), None)
    return rc, K.lib.ag_last_error().decode()


@pytest.mark.parametrize('nl', [2, 5, 8])
def test_a_filled_struct_reaches_the_shape_predicate(nl):
    """B = 65 at S = 1024 is past the chip: AG_ERR_UNSUPPORTED says the struct passed the size and NULL rules; the message
    names B, S, fs, nl and the CU count"""
    rc, msg = call(bwd_args(nl=nl, B=65, S=1024, fs=200, n_cu=208))
    assert rc == _lib.AG_ERR_UNSUPPORTED, msg
    for word in ('ag_gfront_stack_bwd', 'B=65', 'S=1024', 'fs=200', 'nl=%d' % nl, '208 CUs'):
        assert word in msg, msg
    rc, msg = call(bwd_args(nl=nl, B=65, S=1024, fs=200, dh_ext=None, dx_ext=None))      # the external gradients are optional
    assert rc == _lib.AG_ERR_UNSUPPORTED, msg


def test_one_layer_is_not_this_launch():
    rc, msg = call(bwd_args(nl=1))
    assert rc == _lib.AG_ERR_UNSUPPORTED and 'nl=1' in msg, msg
    for nl in (0, 9, -1):
        rc, msg = call(bwd_args(nl=nl))
        assert rc == _lib.AG_ERR_ARG and 'nl = %d' % nl in msg, msg


@pytest.mark.parametrize('off', [-8, 8])
def test_struct_size_mismatch_is_refused(off):
    rc, msg = call(bwd_args(B=65, struct_bytes=SIZE + off))
    assert rc == _lib.AG_ERR_ARG and 'ag_gfront_stack_bwd' in msg and str(SIZE + off) in msg and str(SIZE) in msg, msg
    assert K.lib.ag_gfront_stack_bwd(None, None) == _lib.AG_ERR_ARG


@pytest.mark.parametrize('name,i', [(n, i) for n in TABLES for i in (0, 2)])
def test_a_required_per_layer_pointer_left_null_is_refused(name, i):
    rc, msg = call(bwd_args(nl=3, tables={(name, i): None}))
    assert rc == _lib.AG_ERR_ARG and 'ag_gfront_stack_bwd: %s[%d] is NULL' % (name, i) in msg, msg


@pytest.mark.parametrize('field', ['w_p', 'x', 'dxt', 'ws'])
def test_a_required_pointer_left_null_is_refused(field):
    rc, msg = call(bwd_args(**{field: None}))
    assert rc == _lib.AG_ERR_ARG and 'ag_gfront_stack_bwd: %s is NULL' % field in msg, msg


@pytest.mark.parametrize('name', TABLES)
def test_a_pointer_past_nl_is_refused(name):
    for nl, i in ((2, 2), (2, 7), (7, 7)):
        rc, msg = call(bwd_args(nl=nl, tables={(name, i): PTR}))
        assert rc == _lib.AG_ERR_ARG and '%s[%d] lies past nl' % (name, i) in msg, msg


def test_empty_sequences_short_pitches_and_misaligned_outputs_are_refused():
    for a, word in ((bwd_args(T=0), 'T must'), (bwd_args(T=-3), 'T must'), (bwd_args(ldx=127), 'x row pitch'),
                    (bwd_args(lddx=127), 'dx_ext row pitch'), (bwd_args(ldwx=63), 'w_in[0] row pitch'),
                    (bwd_args(dxt=PTR + 4), '16-byte aligned'), (bwd_args(tables={('dgs', 1): PTR + 8}), '16-byte aligned')):
        rc, msg = call(a)
        assert rc == _lib.AG_ERR_ARG and word in msg, msg
    rc, msg = call(bwd_args(lddx=0, dx_ext=None, B=65, S=1024, fs=200))      # (a pitch of an absent tensor is not looked at)
    assert rc == _lib.AG_ERR_UNSUPPORTED, msg
    rc, msg = call(bwd_args())      # everything right but the workspace: the last check in front of the launch
    assert rc == _lib.AG_ERR_ARG and 'workspace' in msg, msg


def test_struct_layout_and_bindings_are_in_step():
    cls = _lib.FrontStackBwdArgs
    assert SIZE % 8 == 0
    for n, t in cls._fields_:
        if t is not ctypes.c_int32:
            assert getattr(cls, n).offset % 8 == 0, n
    assert [n for n, t in cls._fields_ if t is not ctypes.c_void_p and t not in (ctypes.c_int32, ctypes.c_int64)] == list(TABLES)
    assert all(ctypes.sizeof(t) == 8 * 8 for n, t in cls._fields_ if n in TABLES)
    assert SIZE == 8 + 8 + 5 * 64 + 6 * 8 + 3 * 8 + 6 * 4
    sigs = {'ag_gfront_stack_bwd_ok': (ctypes.c_int, [ctypes.c_int] * 5),
            'ag_gfront_stack_bwd_ws_bytes': (ctypes.c_int64, [ctypes.c_int] * 4),
            'ag_gfront_stack_bwd': (ctypes.c_int, [ctypes.POINTER(cls), ctypes.c_void_p])}
    for sym, sig in sigs.items():
        assert _lib.SIGNATURES[sym] == sig, sym
        assert getattr(K.lib, sym).argtypes == sig[1]
    assert K.lib.ag_abi_version() == 13
    header = open(__file__.rsplit('/tests/', 1)[0] + '/include/audiogan_hip.h').read()
    for sym in ('ag_front_stack_bwd_args', 'int ag_gfront_stack_bwd_ok(int B, int S, int fs, int nl, int n_cu);',
                'int64_t ag_gfront_stack_bwd_ws_bytes(int B, int S, int fs, int nl);',
                'int ag_gfront_stack_bwd(const ag_front_stack_bwd_args* a, void* stream);'):
        assert sym in header, sym
    # the header's fields in the bindings' order
    body = header[header.index('typedef struct ag_front_stack_bwd_args {'):header.index('} ag_front_stack_bwd_args;')]
    import re
    decls = re.sub(r'/\*.*?\*/', '', body[body.index('{') + 1:], flags=re.S).split(';')
    names = [re.sub(r'\[\d+\]', '', d.split()[-1].lstrip('*')) for decl in decls if decl.strip() for d in decl.split(',')]
    assert names == [n for n, _ in cls._fields_], names


# ---- the Python predicate -----------------------------------------------------------------------------------------------
def test_python_predicate_obeys_its_switches(monkeypatch):
    """K.gfront_stack_bwd_ok: PERSIST[0], PERSIST_FRONT_STACK[0], PERSIST_FRONT_STACK_BWD[0], PERSIST_FRONT_BWD[0], a CUDA
    device and the library's rule"""
    monkeypatch.setattr(K, '_n_cu', lambda dev: 256)
    assert K.gfront_stack_bwd_ok(32, 1024, 200, 2, 'cuda') is True
    assert K.gfront_stack_bwd_ok(32, 1024, 200, 2, 'cpu') is False
    assert K.gfront_stack_bwd_ok(33, 1024, 200, 2, 'cuda') is False and K.gfront_stack_bwd_ok(32, 1024, 200, 1, 'cuda') is False
    for sw in (K.PERSIST_FRONT_STACK_BWD, K.PERSIST_FRONT_STACK, K.PERSIST_FRONT_BWD, K.PERSIST):
        old = sw[0]
        sw[0] = False
        try:
            assert K.gfront_stack_bwd_ok(32, 1024, 200, 2, 'cuda') is False
        finally:
            sw[0] = old
    assert K.gfront_stack_bwd_ok(32, 1024, 200, 2, 'cuda') is True
    # the forward's predicate does not look at the backward's switch
    K.PERSIST_FRONT_STACK_BWD[0] = False
    try:
        assert K.gfront_stack_ok(32, 1024, 200, 2, 'cuda') is True
    finally:
        K.PERSIST_FRONT_STACK_BWD[0] = True


def test_front_bwd_persist_false_switches_the_launch_off(monkeypatch):
    """the multi-GPU rule: a generator whose optimiser carries a gradient bucket runs its backward under
    K.front_bwd_persist(False), which must reach this launch as it reaches the one-layer one"""
    monkeypatch.setattr(K, '_n_cu', lambda dev: 256)
    assert K.gfront_stack_bwd_ok(8, 128, 64, 2, 'cuda') is True
    with K.front_bwd_persist(False):
        assert K.gfront_stack_bwd_ok(8, 128, 64, 2, 'cuda') is False
        with K.front_bwd_persist(True):      # (an inner `True` does not switch an outer `False` back on)
            assert K.gfront_stack_bwd_ok(8, 128, 64, 2, 'cuda') is False
    assert K.gfront_stack_bwd_ok(8, 128, 64, 2, 'cuda') is True


# ---- host routing on the torch model of the launch ---------------------------------------------------------------------
HOST_CASES = [dict(id=110, nl=2, S=32, fs=16, B=5, T=4), dict(id=111, nl=3, S=32, fs=8, B=3, T=3), dict(id=112, nl=2, S=32, fs=8, B=2, T=1)]


@pytest.fixture
def routed(monkeypatch):
    """the CPU kernel model with the one-launch backward modelled: returns (calls counter, state: on / mutate)"""
    kernel_model.install(monkeypatch)
    n = collections.Counter()
    state = dict(on=True, mutate=None)

    def bwd(*a_, **k_):
        n.update(['bwd'])
        return BC.stack_bwd_model(*a_, mutate=state['mutate'], **k_)

    def cell_bwd(*a_, _o=K.lstm_cell_bwd, **k_):
        n.update(['cell_bwd'])
        return _o(*a_, **k_)
    monkeypatch.setattr(K, 'gfront_stack_bwd_ok', lambda B, S, fs, nl, dev: nl > 1 and state['on'])
    monkeypatch.setattr(K, 'gfront_stack_bwd_persist', bwd)
    monkeypatch.setattr(K, 'lstm_cell_bwd', cell_bwd)
    return n, state


@pytest.mark.parametrize('slab', [False, True])
@pytest.mark.parametrize('case', HOST_CASES, ids=SC.case_name)
def test_routed_backward_meets_float64(routed, monkeypatch, case, slab):
    """GFrontFn forward + backward with the backward on the modelled launch, against float64 by the bound rule: the wrapper is
    called once per backward pass (the slab form of run_stack_front runs two: frames, then stop logits) and no per-frame cell
    backward runs; with the predicate off the per-frame chain runs and meets the same bounds"""
    n, state = routed
    passes = 2 if slab else 1
    inp, ref, floor = SC.prepared_stack(case)
    got = SC.run_stack_front(monkeypatch, case, inp, 'cpu', slab)
    assert dict(n) == {'bwd': passes}, dict(n)
    SC.check_stack(case, inp, ref, floor, got)
    state['on'] = False
    n.clear()
    got0 = SC.run_stack_front(monkeypatch, case, inp, 'cpu', slab)
    assert n['bwd'] == 0 and n['cell_bwd'] == passes * case['nl'] * case['T'], dict(n)
    SC.check_stack(case, inp, ref, floor, got0)
    for a, b in zip(got['grads'], got0['grads']):
        torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-5)


def test_routed_backward_without_a_stop_gradient_or_without_frames_gradient(routed, monkeypatch):
    """dx alone (no stop head term: dh_ext is None) and ds alone (dx_ext is None) reach the launch as such"""
    from audiogan_amd import ops
    n, state = routed
    case = HOST_CASES[0]
    inp, _, _ = SC.prepared_stack(case)
    seen = []
    monkeypatch.setattr(K, 'gfront_stack_bwd_persist',
                        lambda gates, cs, x, dh_ext, dx_ext, *a_, **k_: (seen.append((dh_ext is None, dx_ext is None)),
                                                                        BC.stack_bwd_model(gates, cs, x, dh_ext, dx_ext, *a_, **k_))[1])
    for which in ('x', 's'):
        front = SC.build_front(case, inp, 'cpu')
        zc = inp['zc'].clone().requires_grad_(True)
        x, s = ops.GFrontFn.apply(zc, front, *front.group.params())
        ((x * inp['gx']).sum() if which == 'x' else (s * inp['gs']).sum()).backward()
        assert zc.grad is not None and bool(torch.isfinite(zc.grad).all())
    assert seen == [(True, False), (False, True)], seen


def test_switch_off_the_wrapper_is_never_called(monkeypatch):
    """the REAL predicate (off CUDA, and with PERSIST_FRONT_STACK_BWD[0] = False): GFrontFn.backward keeps the per-frame chain"""
    kernel_model.install(monkeypatch)

    def boom(*a_, **k_):
        raise AssertionError('the one-launch backward was called with its switch off')
    monkeypatch.setattr(K, 'gfront_stack_bwd_persist', boom)
    case = dict(id=113, nl=2, S=128, fs=8, B=2, T=2)
    inp = SC.make_stack_inputs(case)
    assert not K.gfront_stack_bwd_ok(2, 128, 8, 2, 'cpu')
    SC.run_stack_front(monkeypatch, case, inp, 'cpu')
    monkeypatch.setattr(K, '_n_cu', lambda dev: 256)
    K.PERSIST_FRONT_STACK_BWD[0] = False
    try:
        assert not K.gfront_stack_bwd_ok(2, 128, 8, 2, 'cuda')
        SC.run_stack_front(monkeypatch, case, inp, 'cpu')
    finally:
        K.PERSIST_FRONT_STACK_BWD[0] = True


# ---- the checkers reject wrong launches --------------------------------------------------------------------------------
MUT_CASE = dict(id=114, nl=3, S=32, fs=16, B=4, T=4)


def _direct(mutate):
    inp, _, _ = SC.prepared_stack(MUT_CASE)
    h = BC.cpu_history(MUT_CASE, inp)
    chain = BC.stack_bwd_chain(h['gates'], h['cs'], h['x'], h['dh_ext'], h['dx_ext'], h['whh'], h['w_in'], h['wx'], h['wp'])
    floor = BC.direct_errors(chain, BC.run_direct(BC.stack_bwd_model, h))
    got = BC.run_direct(lambda *a_: BC.stack_bwd_model(*a_, mutate=mutate), h)
    return chain, floor, got


def test_the_chain_is_autograd_of_the_float64_front():
    """stack_bwd_chain on the float64 reference's own history gives the reference's dzc (= dg_0 W_ih_0[:, fs:]): the chain is the
    backward of ref_stack_front, not a second opinion of this file"""
    case = MUT_CASE
    inp, ref, _ = SC.prepared_stack(case)
    nl, S, fs, B, T = case['nl'], case['S'], case['fs'], case['B'], case['T']
    d = lambda t: t.double()      # noqa: E731
    inp64 = dict(inp, vg=[(d(v), d(g)) for v, g in inp['vg']], zc=d(inp['zc']), gx=d(inp['gx']), gs=d(inp['gs']))
    lw, pw, pb, sw, sb = BC.effective_weights(inp64, nl)
    # the history in float64, by the forward model run in float64
    torch.set_default_dtype(torch.float64)
    try:
        h = BC.cpu_history(case, inp64)
    finally:
        torch.set_default_dtype(torch.float32)
    dgs, dxt = BC.stack_bwd_chain(h['gates'], h['cs'], h['x'], h['dh_ext'], h['dx_ext'], h['whh'], h['w_in'], h['wx'], h['wp'])
    dzc = (dgs[0].view(T * B, 4 * S) @ lw[0][0][:, fs:]).view(T, B, -1)
    assert RC.err_of(dzc, ref['dzc']) < 1e-10


def test_checker_accepts_the_model():
    chain, floor, got = _direct(None)
    ratios = BC.check_direct('model', chain, floor, got, again=got)
    assert set(ratios) == {'dgs[0]', 'dgs[1]', 'dgs[2]', 'dxt'}
    assert all(r <= 1.0 for r in ratios.values())


@pytest.mark.parametrize('mutate', ['input_next', 'ext_l0', 'rec_wih', 'no_dc', 'proj_all'])
def test_checker_rejects_a_wrong_chain(mutate):
    chain, floor, got = _direct(mutate)
    with pytest.raises(AssertionError, match='out of bound'):
        BC.check_direct(mutate, chain, floor, got)


def test_checker_rejects_a_store_past_the_last_row():
    chain, floor, got = _direct('row_past_B')
    with pytest.raises(AssertionError, match='guard frame'):
        BC.check_direct('row_past_B', chain, floor, got)
    got['frames_ok'] = True       # ... and nothing else is wrong with that launch
    BC.check_direct('row_past_B', chain, floor, got)


@pytest.mark.parametrize('mutate', ['input_next', 'ext_l0', 'rec_wih', 'no_dc', 'proj_all'])
def test_end_to_end_checker_rejects_a_wrong_chain(routed, monkeypatch, mutate):
    """the same mutants through GFrontFn and SC.check_stack, the checker of the GPU test's end-to-end part"""
    n, state = routed
    inp, ref, floor = SC.prepared_stack(MUT_CASE)
    state['mutate'] = mutate
    got = SC.run_stack_front(monkeypatch, MUT_CASE, inp, 'cpu')
    assert n['bwd'] == 1 and n['cell_bwd'] == 0
    with pytest.raises(AssertionError, match='out of bound'):
        SC.check_stack(MUT_CASE, inp, ref, floor, got)
