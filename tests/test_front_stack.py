"""Stacked LSTM fronts in one launch (ag_gfront_stack_fwd), everything that needs no GPU: the shape predicate and the workspace
size of libaudiogan_hip.so, what the launcher refuses before any HIP call, the host routing of recurrent.GFrontFn /
front_sample / Generator.front_is_persistent on a torch model of the launch's contract (tests/stacked_front_cases.py), and the
checkers of the GPU test shown to reject subtly wrong launches.  The real launch: tests/test_gpu_front_stack.py (-m gpu)."""
import collections
import ctypes

import pytest
import torch

import audiogan_amd.kernels as K
from audiogan_amd import _lib
from tests import kernel_model
from tests import stacked_front_cases as SC

N_CU = SC.N_CU


# ---- the shape predicate and the workspace ----------------------------------------------------------------------------
@pytest.mark.parametrize('case', SC.CASES, ids=SC.case_name)
def test_every_case_takes_the_stacked_launch(case):
    assert K.lib.ag_gfront_stack_ok(case['B'], case['S'], case['fs'], case['nl'], N_CU) == 1


@pytest.mark.parametrize('nl,S,fs,B', SC.REFUSED)
def test_shapes_outside_the_rule_keep_the_per_frame_path(nl, S, fs, B):
    assert K.lib.ag_gfront_stack_ok(B, S, fs, nl, N_CU) == 0


def test_co_residency_counts_every_layer():
    ok = K.lib.ag_gfront_stack_ok
    assert ok(32, 1024, 200, 2, 256) == 1 and ok(32, 1024, 200, 2, 255) == 0        # 2 * 1 * 128 workgroups
    assert ok(32, 1024, 200, 2, 304) == 1 and ok(32, 1024, 200, 3, 512) == 0        # at most 256, whatever the chip has
    assert ok(64, 128, 64, 2, 64) == 1 and ok(64, 128, 64, 2, 63) == 0              # 2 * 2 * 16
    assert ok(0, 128, 64, 2, 256) == 0 and ok(65, 128, 64, 2, 256) == 0
    for B in (1, 32, 64):
        assert ok(B, 128, 64, 1, 256) == 0 and ok(B, 128, 64, 0, 256) == 0          # one layer stays on ag_gfront_fwd


def test_workspace_grows_by_one_h_buffer_per_layer():
    ws = K.lib.ag_gfront_stack_ws_bytes
    for B, S, w in ((32, 1024, 256), (64, 1024, 256), (33, 128, 64)):
        nrt = (B + 31) // 32
        for nl in range(2, 8):
            assert ws(B, S, 8, nl + 1) - ws(B, S, 8, nl) == 2 * nrt * 32 * S * 4
        assert ws(B, S, 8, 2) == 256 + 8192 + 2 * nrt * 32 * (2 * S + w) * 4
    assert ws(32, 1024, 200, 2) == ws(32, 1024, 256, 2) == ws(1, 1024, 8, 2)        # the padded panel width whatever fs is
    assert ws(40, 128, 40, 3) == ws(40, 128, 64, 3)
    assert ws(32, 1024, 200, 2) - K.lib.ag_gfront_persist_ws_bytes(32, 1024, 200) == 2 * 32 * 1024 * 4


# ---- the argument struct: what the launcher refuses, before any HIP call -----------------------------------------------
# Every case here fails validation, so nothing is enqueued and no pointer is followed: the fields point at one small host
# buffer, and ws_bytes = 0 would stop a call that slipped through the rule under test at the workspace check.
_HOST = ctypes.create_string_buffer(64 + 16)
PTR = (ctypes.addressof(_HOST) + 15) & ~15
SIZE = ctypes.sizeof(_lib.FrontStackArgs)
GEN_FIELDS = ('w_s', 'b_s', 'u', 's', 'first', 't_run')
TABLES = ('gates', 'hs', 'cs', 'w_hh', 'w_in', 'bias')


def stack_args(gen, nl=2, B=4, S=128, fs=64, T=2, tables=None, **over):
    used = ['w_p', 'b_p', 'x', 'ws'] + (list(GEN_FIELDS) if gen else ['xt'])
    kw = dict({n: PTR for n in used}, struct_bytes=SIZE, gen=gen, nl=nl, ldx=T * fs, lds=T, ldwx=fs, ws_bytes=0, T=T, B=B, S=S,
              fs=fs, n_cu=N_CU)
    kw.update(over)
    a = _lib.FrontStackArgs(**kw)
    n = max(min(nl, 8), 0)
    fill = dict(gates=range(1 if gen else n), hs=range(0 if gen else n), cs=range(0 if gen else n), w_hh=range(n), w_in=range(n),
                bias=range(1, n))
    for name, idx in fill.items():
        for i in idx:
            getattr(a, name)[i] = PTR
    for (name, i), v in (tables or {}).items():
        getattr(a, name)[i] = v
    return a


def call(a):
    rc = K.lib.ag_gfront_stack_fwd(ctypes.byref(a), None)
    return rc, K.lib.ag_last_error().decode()


@pytest.mark.parametrize('gen', [0, 1])
@pytest.mark.parametrize('nl', [2, 5, 8])
def test_a_filled_struct_reaches_the_shape_predicate(gen, nl):
    """B = 65 is past the batch limit: AG_ERR_UNSUPPORTED says the struct passed the size, mode and NULL rules; the message
    names B, S, fs, nl and the CU count"""
    rc, msg = call(stack_args(gen, nl=nl, B=65, S=1024, fs=200, n_cu=208))
    assert rc == _lib.AG_ERR_UNSUPPORTED, msg
    for word in ('ag_gfront_stack_fwd', 'B=65', 'S=1024', 'fs=200', 'nl=%d' % nl, '208 CUs'):
        assert word in msg, msg


@pytest.mark.parametrize('gen', [0, 1])
def test_one_layer_is_not_this_launch(gen):
    rc, msg = call(stack_args(gen, nl=1))
    assert rc == _lib.AG_ERR_UNSUPPORTED and 'nl=1' in msg, msg
    for nl in (0, 9, -1):
        rc, msg = call(stack_args(gen, nl=nl))
        assert rc == _lib.AG_ERR_ARG and 'nl = %d' % nl in msg, msg


@pytest.mark.parametrize('off', [-8, 8])
@pytest.mark.parametrize('gen', [0, 1])
def test_struct_size_mismatch_is_refused(gen, off):
    rc, msg = call(stack_args(gen, B=65, struct_bytes=SIZE + off))
    assert rc == _lib.AG_ERR_ARG and 'ag_gfront_stack_fwd' in msg and str(SIZE + off) in msg and str(SIZE) in msg, msg
    assert K.lib.ag_gfront_stack_fwd(None, None) == _lib.AG_ERR_ARG


@pytest.mark.parametrize('gen,name,i', [(0, 'gates', 0), (0, 'gates', 1), (0, 'hs', 2), (0, 'cs', 0), (0, 'w_hh', 1), (0, 'w_in', 0),
                                        (0, 'w_in', 2), (0, 'bias', 1), (1, 'gates', 0), (1, 'w_hh', 2), (1, 'bias', 2)])
def test_a_required_per_layer_pointer_left_null_is_refused(gen, name, i):
    rc, msg = call(stack_args(gen, nl=3, tables={(name, i): None}))
    assert rc == _lib.AG_ERR_ARG and 'ag_gfront_stack_fwd: %s[%d] is NULL' % (name, i) in msg, msg


@pytest.mark.parametrize('gen,field', [(0, 'w_p'), (0, 'x'), (1, 'b_p'), (1, 'u'), (1, 't_run'), (1, 'first'), (0, 'ws')])
def test_a_required_pointer_left_null_is_refused(gen, field):
    rc, msg = call(stack_args(gen, **{field: None}))
    assert rc == _lib.AG_ERR_ARG and 'ag_gfront_stack_fwd: %s is NULL' % field in msg, msg


@pytest.mark.parametrize('gen', [0, 1])
@pytest.mark.parametrize('name', TABLES)
def test_a_pointer_past_nl_is_refused(gen, name):
    for nl, i in ((2, 2), (2, 7), (7, 7)):
        rc, msg = call(stack_args(gen, nl=nl, tables={(name, i): PTR}))
        assert rc == _lib.AG_ERR_ARG and '%s[%d] lies past nl' % (name, i) in msg, msg


@pytest.mark.parametrize('name,i', [('gates', 1), ('hs', 0), ('hs', 1), ('cs', 0), ('cs', 1)])
def test_history_pointers_in_generation_mode_are_refused(name, i):
    rc, msg = call(stack_args(1, tables={(name, i): PTR}))
    assert rc == _lib.AG_ERR_ARG and 'ag_gfront_stack_fwd: %s[%d] is not used' % (name, i) in msg, msg
    rc, msg = call(stack_args(1, xt=PTR))
    assert rc == _lib.AG_ERR_ARG and 'ag_gfront_stack_fwd: xt is not used' in msg, msg


@pytest.mark.parametrize('gen', [0, 1])
def test_layer_0_has_no_bias_vector_and_modes_do_not_mix(gen):
    rc, msg = call(stack_args(gen, tables={('bias', 0): PTR}))
    assert rc == _lib.AG_ERR_ARG and 'ag_gfront_stack_fwd: bias[0] is not used' in msg, msg
    if not gen:
        for field in GEN_FIELDS:
            rc, msg = call(stack_args(0, **{field: PTR}))
            assert rc == _lib.AG_ERR_ARG and '%s is not used' % field in msg, msg
        rc, msg = call(stack_args(0, B=65, xt=None))          # xt stays optional in training
        assert rc == _lib.AG_ERR_UNSUPPORTED, msg


def test_bad_modes_and_empty_sequences_are_refused():
    for a, word in ((stack_args(2), 'gen'), (stack_args(-1), 'gen'), (stack_args(0, T=0), 'T must'), (stack_args(1, T=0), 'T must'),
                    (stack_args(0, ldx=127), 'x row pitch'), (stack_args(1, lds=1), 's row pitch')):
        rc, msg = call(a)
        assert rc == _lib.AG_ERR_ARG and word in msg, msg


def test_struct_layout_and_bindings_are_in_step():
    cls = _lib.FrontStackArgs
    assert SIZE % 8 == 0
    for n, t in cls._fields_:
        if t is not ctypes.c_int32:
            assert getattr(cls, n).offset % 8 == 0, n
    assert [n for n, t in cls._fields_ if t is not ctypes.c_void_p and t not in (ctypes.c_int32, ctypes.c_int64)] == list(TABLES)
    assert all(ctypes.sizeof(t) == 8 * 8 for n, t in cls._fields_ if n in TABLES)
    for sym in ('ag_gfront_stack_ok', 'ag_gfront_stack_ws_bytes', 'ag_gfront_stack_fwd'):
        assert sym in _lib.SIGNATURES
    assert K.lib.ag_abi_version() == 13
    header = open(__file__.rsplit('/tests/', 1)[0] + '/include/audiogan_hip.h').read()
    for sym in ('ag_front_stack_args', 'int ag_gfront_stack_ok(int B, int S, int fs, int nl, int n_cu);',
                'int64_t ag_gfront_stack_ws_bytes(int B, int S, int fs, int nl);',
                'int ag_gfront_stack_fwd(const ag_front_stack_args* a, void* stream);'):
        assert sym in header, sym


def test_python_predicate_obeys_its_switches(monkeypatch):
    """K.gfront_stack_ok: PERSIST[0], PERSIST_FRONT_STACK[0], a CUDA device and the library's rule, all four"""
    monkeypatch.setattr(K, '_n_cu', lambda dev: 256)
    assert K.PERSIST_FRONT_STACK == [True]
    assert K.gfront_stack_ok(32, 1024, 200, 2, 'cuda') is True
    assert K.gfront_stack_ok(32, 1024, 200, 2, 'cpu') is False
    assert K.gfront_stack_ok(33, 1024, 200, 2, 'cuda') is False and K.gfront_stack_ok(32, 1024, 200, 1, 'cuda') is False
    for sw in (K.PERSIST_FRONT_STACK, K.PERSIST):
        old = sw[0]
        sw[0] = False
        try:
            assert K.gfront_stack_ok(32, 1024, 200, 2, 'cuda') is False
        finally:
            sw[0] = old
    assert K.gfront_stack_ok(32, 1024, 200, 2, 'cuda') is True


# ---- host routing on the torch model of the launch ---------------------------------------------------------------------
HOST_CASES = [dict(id=100, nl=2, S=32, fs=16, B=5, T=4), dict(id=101, nl=3, S=32, fs=8, B=3, T=3)]


@pytest.fixture
def routed(monkeypatch):
    """the CPU kernel model with the stacked launch modelled: returns (calls counter, switch(on) for the predicate)"""
    kernel_model.install(monkeypatch)
    n = collections.Counter()
    state = dict(on=True, mutate=None)

    def fwd(*a_, **k_):
        n.update(['fwd'])
        return SC.stack_fwd_model(*a_, mutate=state['mutate'], **k_)

    def gen(*a_, **k_):
        n.update(['gen'])
        return SC.stack_gen_model(*a_, mutate=state['mutate'], **k_)
    monkeypatch.setattr(K, 'gfront_stack_ok', lambda B, S, fs, nl, dev: nl > 1 and state['on'])
    monkeypatch.setattr(K, 'gfront_stack_fwd_persist', fwd)
    monkeypatch.setattr(K, 'gfront_stack_gen_persist', gen)
    return n, state


def _spy_history(monkeypatch):
    """records what GFrontFn._bwd_frames is handed: (gates, hs, cs) lists"""
    from audiogan_amd import recurrent
    seen = []
    orig = recurrent.GFrontFn._bwd_frames

    def spy(T, B, fs, S, nl, x, dx, ds, gates, cs, lw, wx, pw, sw, hs, dws):
        seen.append(dict(gates=[g.clone() for g in gates], hs=[h.clone() for h in hs], cs=[c.clone() for c in cs], x=x.clone()))
        return orig(T, B, fs, S, nl, x, dx, ds, gates, cs, lw, wx, pw, sw, hs, dws)
    monkeypatch.setattr(recurrent.GFrontFn, '_bwd_frames', staticmethod(spy))
    return seen


@pytest.mark.parametrize('case', HOST_CASES, ids=SC.case_name)
def test_routed_forward_and_backward_equal_the_per_frame_path(routed, monkeypatch, case):
    """GFrontFn on the modelled launch and on the per-frame path, EACH against float64 by the bound rule; the history the
    per-frame backward reads is the one the launch wrote (and the per-frame path's own, to fp32 rounding)"""
    n, state = routed
    seen = _spy_history(monkeypatch)
    inp, ref, floor = SC.prepared_stack(case)
    got = {}
    for on in (True, False):
        state['on'] = on
        n.clear()
        got[on] = SC.run_stack_front(monkeypatch, case, inp, 'cpu')
        assert dict(n) == ({'fwd': 1} if on else {}), dict(n)
        SC.check_stack(case, inp, ref, floor, got[on])
    a, b = seen
    for k in ('gates', 'hs', 'cs'):
        for l in range(case['nl']):
            torch.testing.assert_close(a[k][l], b[k][l], rtol=1e-5, atol=1e-6, msg='%s[%d]' % (k, l))
    assert all(not bool(c[0].any()) for c in a['cs'])
    torch.testing.assert_close(got[True]['x'], got[False]['x'], rtol=1e-5, atol=1e-6)


def test_switch_off_nothing_calls_the_new_wrappers(monkeypatch):
    """the REAL predicate with PERSIST_FRONT_STACK[0] = False (its switch logic: test_python_predicate_obeys_its_switches):
    GFrontFn and front_sample take the per-frame path"""
    from audiogan_amd.recurrent import front_sample
    kernel_model.install(monkeypatch)

    def boom(*a_, **k_):
        raise AssertionError('the stacked launch was called with its switch off')
    monkeypatch.setattr(K, 'gfront_stack_fwd_persist', boom)
    monkeypatch.setattr(K, 'gfront_stack_gen_persist', boom)
    case = dict(id=102, nl=2, S=128, fs=8, B=2, T=2)
    inp = SC.make_stack_inputs(case)
    front = SC.build_front(case, inp, 'cpu')
    old = K.PERSIST_FRONT_STACK[0]
    K.PERSIST_FRONT_STACK[0] = False
    try:
        assert not K.gfront_stack_ok(2, 128, 8, 2, 'cpu')
        from audiogan_amd import ops
        with torch.no_grad():
            ops.GFrontFn.apply(inp['zc'], front, *front.group.params())
            x, s, first, t_run = front_sample(front, inp['zc'], torch.ones(2, 2))
        assert t_run is None
    finally:
        K.PERSIST_FRONT_STACK[0] = old


@pytest.mark.parametrize('frames', [[2, 0, 4, None, 1], [2, 0, 3, 1, 1], [0, 0, 0, 0, 0]])
def test_front_sample_returns_the_launches_first_and_t_run(routed, frames):
    from audiogan_amd.recurrent import front_sample
    n, state = routed
    case = dict(id=103, nl=2, S=32, fs=16, B=5, T=6)
    inp = SC.make_stack_inputs(case)
    front = SC.build_front(case, inp, 'cpu')
    T = case['T']
    u = torch.ones(T, 5)
    for b, k in enumerate(frames):
        if k is not None:
            u[k, b] = 0.0
    want = torch.tensor([T if k is None else k + 1 for k in frames])
    with torch.no_grad():
        x, s, first, t_run = front_sample(front, inp['zc'], u)
    assert dict(n) == {'gen': 1}
    assert first.dtype == torch.int64 and torch.equal(first, want)
    assert int(t_run) == min(T, int(want.max()) + SC.GEN_LAG)
    # the frames run are the training front's
    state['on'] = False
    with torch.no_grad():
        x0, s0, first0, none = front_sample(front, inp['zc'], u)
    assert none is None and torch.equal(first0, want)
    k = int(t_run)
    torch.testing.assert_close(x[:, :k * 16], x0[:, :k * 16], rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(s[:, :k], s0[:, :k], rtol=1e-5, atol=1e-6)


def test_generator_front_is_persistent_follows_the_new_predicate(monkeypatch):
    import audiogan_amd as A
    asked = []
    monkeypatch.setattr(K, 'gfront_persist_ok', lambda *a_: asked.append(('one',) + a_) or True)
    answer = [True]
    monkeypatch.setattr(K, 'gfront_stack_ok', lambda *a_: asked.append(('stack',) + a_) or answer[0])
    cfg = dict(frame_size=32, embed_size=8, noise_size=8, state_size=64, struct=[[17, 8, 16, 8], [9, 4, 16, 8]])
    g2, g1 = A.Generator(num_layers=2, **cfg), A.Generator(num_layers=1, **cfg)
    assert g2.front_is_persistent(4, 'cpu') is True
    answer[0] = False
    assert g2.front_is_persistent(4, 'cpu') is False
    assert asked == [('stack', 4, 64, 32, 2, 'cpu')] * 2
    del asked[:]
    assert g1.front_is_persistent(4, 'cpu') is True and asked == [('one', 4, 64, 32, 'cpu')]


# ---- the checkers reject wrong launches --------------------------------------------------------------------------------
MUT_CASE = dict(id=104, nl=3, S=32, fs=16, B=4, T=4)


def test_the_float64_statement_is_the_oracles_generator():
    """ref_stack_front against the oracle's Generator front (torch LSTMCells) on one case: frames and stop logits"""
    from oracle import audiogan_oracle as O
    torch.manual_seed(3)
    cfg = dict(frame_size=16, embed_size=8, noise_size=8, state_size=32, struct=[[17, 8, 16, 8]])
    go = O.Generator(num_layers=2, **cfg)
    sd = go.state_dict()
    names = ['rnn.%d.%s' % (l, n) for l in range(2) for n in ('weight_ih', 'weight_hh', 'bias_ih', 'bias_hh')] + \
        ['proj.weight', 'proj.bias', 'stopper.weight', 'stopper.bias']
    key = lambda n, part: [k for k in sd if k.startswith(n.rsplit('.', 1)[0]) and k.endswith(n.rsplit('.', 1)[1] + '_' + part)]     # noqa: E731
    vg = []
    for n in names:
        (kv,), (kg,) = key(n, 'v'), key(n, 'g')
        vg.append((sd[kv], sd[kg]))
    B, T = 3, 4
    z, c = torch.randn(B, T, 8), torch.randn(B, 8)
    zc = torch.cat([z, c.unsqueeze(1).expand(B, T, 8)], 2).transpose(0, 1).contiguous()
    ref = SC.ref_stack_front(2, zc, vg, torch.zeros(B, T * 16), torch.ones(B, T))
    stop = torch.zeros(B, T, dtype=torch.long)
    with torch.no_grad():
        # the oracle's front alone: its frames before the conv trunk are not returned, so compare the stop logits (they see
        # every layer, the feedback and both heads' inputs) over all frames
        _, so, _, _ = go(z=z, c=c, stop=stop)
    torch.testing.assert_close(ref['s'].float(), so, rtol=1e-4, atol=1e-5)


def _routed_got(monkeypatch, state, mutate):
    inp, ref, floor = SC.prepared_stack(MUT_CASE)
    state['mutate'] = mutate
    return inp, ref, floor, SC.run_stack_front(monkeypatch, MUT_CASE, inp, 'cpu')


def test_checker_accepts_the_model(routed, monkeypatch):
    n, state = routed
    inp, ref, floor, got = _routed_got(monkeypatch, state, None)
    ratios = SC.check_stack(MUT_CASE, inp, ref, floor, got, again=got)
    assert set(ratios) >= {'x', 's', 'dzc', 'dl2.w_ih_v.l2', 'dl1.b_hh_g.elem', 'dl0.b_ih_v.elem', 'dstop.w_g.l2', 'dproj.b_g.elem'}
    assert len(ratios) == 3 + 3 * (2 * 4 + 2 * 3) + (2 * 4 + 2 * 3) - 0      # x s dzc; per tensor .l2 + .elem, a bias dv: .elem only
    assert n['fwd'] == 1


@pytest.mark.parametrize('mutate', ['proj_from_l0', 'lower_prev', 'no_upper_bias'])
def test_checker_rejects_a_wrong_training_launch(routed, monkeypatch, mutate):
    n, state = routed
    inp, ref, floor, got = _routed_got(monkeypatch, state, mutate)
    with pytest.raises(AssertionError, match='out of bound'):
        SC.check_stack(MUT_CASE, inp, ref, floor, got)
    # and the mutant IS the mutated statement: the same checker accepts it against the mutated float64 reference
    mref = SC.ref_stack_front(3, inp['zc'], inp['vg'], inp['gx'], inp['gs'], mutate=mutate)
    m32 = SC.ref_stack_front(3, inp['zc'], inp['vg'], inp['gx'], inp['gs'], dtype=torch.float32, mutate=mutate)
    SC.check_stack(MUT_CASE, inp, mref, dict(x=SC.err_of(m32['x'], mref['x'])), got, only=('x',))


@pytest.mark.parametrize('mutate', [None] + list(SC.MUTANTS))
def test_checker_on_the_generation_mode(routed, mutate):
    """u = 1: the generation launch's frames and logits over all T frames against float64; every mutant fails, the stop head
    on the previous frame's h among them (frames right, logits wrong)"""
    from audiogan_amd.recurrent import front_sample
    n, state = routed
    inp, ref, floor = SC.prepared_stack(MUT_CASE)
    front = SC.build_front(MUT_CASE, inp, 'cpu')
    state['mutate'] = mutate
    T, B = MUT_CASE['T'], MUT_CASE['B']
    with torch.no_grad():
        x, s, first, t_run = front_sample(front, inp['zc'], torch.ones(T, B))
    assert int(t_run) == T and bool((first == T).all()) and dict(n) == {'gen': 1}
    got = dict(x=x, s=s)
    if mutate is None:
        SC.check_stack(MUT_CASE, inp, ref, floor, got, only=('x', 's'))
    else:
        with pytest.raises(AssertionError, match='out of bound'):
            SC.check_stack(MUT_CASE, inp, ref, floor, got, only=('x', 's'))
        if mutate == 'stop_prev':
            SC.check_stack(MUT_CASE, inp, ref, floor, got, only=('x',))
