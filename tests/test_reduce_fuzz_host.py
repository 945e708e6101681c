"""No GPU: the parts of the deferred-reduction sequence fuzz (tests/reduce_cases.py, tests/test_reduce_fuzz.py) that can be
pinned on the host, so that the GPU test is not the first thing to exercise them.

  - model(seq) / trace(seq) against expectations written out by hand: the 40 / 41 boundary of the table, each clash pair, the
    adjacency case, the mixed direct / two-stage writes, the scopes;
  - coverage() over the pinned lists, and that it fails when a class is taken out;
  - the REAL ``kernels.deferred_reduces``, ``_immediate``, ``flush_reduces``, ``_bind_ws`` and the ``hold`` logic of gemm /
    col_sum / gemm_h with ``kernels.lib`` replaced by a recorder that answers 0: the sequence of ag_defer_reduces modes and
    ag_flush_reduces calls for every role and error path, and ``_DEFER`` at rest after each;
  - both passes of a handful of sequences through the CPU kernel model: the references and the runner agree, and the checker
    rejects a subtly wrong reduction.
"""
import pytest
import torch

from tests import kernel_model as KM
from tests import reduce_cases as RC


def _find(seqs, name):
    return [q for q in seqs if q.name == name][0]


# ---------------------------------------------------------------------------------------------------------------------
# the model of the recording rules
# ---------------------------------------------------------------------------------------------------------------------
def test_restated_forms_of_the_stage_makers():
    q = RC.Seq('forms', 'x')
    for Z in RC.Z_SWEEP:
        for N in (8, 7, 4, 3):
            s = RC.st_col(q, 'z%d n%d' % (Z, N), Z, N)
            assert RC.slabs(s) == Z and RC.two_stage(s) and RC.vec_stage(q, s) == (N % 4 == 0)
    assert not RC.two_stage(RC.st_col(q, 'direct', 0, 8)) and not RC.two_stage(q.step('col_sum', 'direct', M=16, N=8))
    assert RC.two_stage(q.step('col_sum', 'direct', M=17, N=8))
    assert RC.slabs(RC.st_chan(q, 'c2', 5, True)) == 2 and RC.slabs(RC.st_chan(q, 'c1', 5, False)) == 1
    assert RC.vec_stage(q, RC.st_conv(q, 'wv', True)) and not RC.vec_stage(q, RC.st_conv(q, 'ws', False))
    for kind in ('gemm', 'gemm_h'):
        for form, vec in (('c', True), ('pv', True), ('ps', False)):
            s = RC.st_gemm(q, '%s %s' % (kind, form), form, True, kind=kind)
            d = q.dests[s.dest]
            assert RC.two_stage(s) and RC.slabs(s) == 4 and RC.vec_stage(q, s) == vec and (d.ld == d.ncol) == (form == 'c')
            assert not RC.two_stage(RC.st_gemm(q, '%s %s direct' % (kind, form), form, False, kind=kind))


def test_model_table_boundary_40_41():
    seqs = RC.table_sequences()
    t40 = RC.trace(_find(seqs, 'table 40'))
    assert [t['flush'] for t in t40 if t['flush']] == ['exit']
    assert t40[-2]['final'] == frozenset() and len(t40[-2]['pending']) == 40 and t40[-1]['final'] == frozenset(t40[-2]['pending'])
    q = _find(seqs, 'table 41')
    t41 = RC.trace(q)
    names = list(q.dests)
    idx = dict((it[1], i) for i, it in enumerate(q.items) if not isinstance(it, RC.Step))
    assert t41[idx['after 40']]['final'] == frozenset(names[40:])             # before stage 41 every one issued is pending
    assert t41[idx['after 41']]['final'] == frozenset(names[:40]) and t41[idx['after 41']]['pending'] == (names[40],)
    step41 = [i for i, s in q.steps()][40]
    assert t41[step41]['flush'] == 'table' and t41[step41]['slot'] == 0 and [t['flush'] for t in t41].count('table') == 1
    q = _find(seqs, 'table 81')
    t81 = RC.trace(q)
    names = list(q.dests)
    idx = dict((it[1], i) for i, it in enumerate(q.items) if not isinstance(it, RC.Step))
    assert t81[idx['after 80']]['final'] == frozenset(names[:40] + names[80:]) and len(t81[idx['after 80']]['pending']) == 40
    assert t81[idx['after 81']]['final'] == frozenset(names[:80]) and [t['flush'] for t in t81].count('table') == 2
    for n in (1, 2, 39):
        tr = RC.trace(_find(seqs, 'table %d' % n))
        assert len(tr[-2]['pending']) == n and [t['flush'] for t in tr if t['flush']] == ['exit']
    assert RC.model(q) == [t['final'] for t in t81]


def test_model_clash_pairs_and_adjacency():
    seqs = RC.clash_sequences()
    for a0, a1 in RC.ACC_PAIRS:
        tr = RC.trace(_find(seqs, 'same output acc %d/%d' % (a0, a1)))
        # items: step, check, step, check
        assert [t['flush'] for t in tr] == [None, None, 'clash', None, 'exit']
        assert tr[1]['final'] == frozenset() and tr[1]['applied'] == ()
        assert tr[3]['final'] == frozenset() and tr[3]['applied'] == (0,) and tr[4]['applied'] == (0, 2)
    tr = RC.trace(_find(seqs, 'column blocks of one matrix'))                 # spans overlap whole: flush
    assert [t['flush'] for t in tr] == [None, 'clash', None, 'exit'] and tr[2]['final'] == frozenset(['left'])
    tr = RC.trace(_find(seqs, 'adjacent vectors of one buffer'))              # disjoint spans: both stay pending
    assert [t['flush'] for t in tr] == [None, None, None, 'exit'] and tr[2]['final'] == frozenset() and tr[2]['pending'] == ('lo', 'hi')
    tr = RC.trace(_find(seqs, 'vector inside the span of a pitched block'))
    assert [t['flush'] for t in tr] == [None, 'clash', None, 'exit'] and tr[2]['final'] == frozenset(['blk'])
    a, b = RC.Dest('f', 0, 8, 8, 24), RC.Dest('f', 8, 8, 12, 24)
    assert RC.span(a) == 7 * 24 + 8 and RC.overlap(a, b) and RC.overlap(b, a)
    assert not RC.overlap(RC.Dest('f', 0, 1, 8, 8), RC.Dest('f', 8, 1, 7, 7)) and RC.overlap(RC.Dest('f', 0, 1, 9, 9), RC.Dest('f', 8, 1, 7, 7))
    assert not RC.overlap(a, RC.Dest('g', 0, 8, 8, 24))


def test_model_mixed_writes():
    seqs = RC.mixed_sequences()
    for kind in ('col_sum', 'gemm', 'gemm_h', 'channel_sum'):
        for defer2 in ((True, False) if kind != 'channel_sum' else (True,)):
            q = _find(seqs, 'mixed %s acc 1/1 two-stage then direct, second defer=%s' % (kind, defer2))
            tr = RC.trace(q)                                                  # items: step, check, step, check
            assert tr[0]['recorded'] and tr[1]['final'] == frozenset() and tr[1]['applied'] == ()
            assert tr[2]['flush'] == 'direct' and not tr[2]['recorded'] and tr[3]['final'] == frozenset(['out'])
            assert tr[3]['applied'] == (0, 2)                                 # the recorded stage lands FIRST
            old = RC.trace(q, flush_before_direct=False)                      # what the library did before: opposite order
            assert old[3]['applied'] == (2,) and old[4]['applied'] == (2, 0)
            q = _find(seqs, 'mixed %s acc 1/1 direct then two-stage, second defer=%s' % (kind, defer2))
            tr = RC.trace(q)
            assert not tr[0]['recorded'] and tr[1]['final'] == frozenset(['out']) and tr[1]['applied'] == (0,)
            assert tr[2]['recorded'] == defer2 and tr[2]['flush'] is None
            assert tr[3]['final'] == (frozenset() if defer2 else frozenset(['out'])) and tr[4]['applied'] == (0, 2)


def test_model_scopes():
    seqs = RC.scope_sequences()
    q = _find(seqs, 'outer scope, two inner blocks')
    tr = RC.trace(q)
    idx = dict((it[1], i) for i, it in enumerate(q.items) if not isinstance(it, RC.Step) and it[0] == 'check')
    rec = dict((q.items[i].dest, tr[i]['recorded']) for i, _ in q.steps())
    assert rec == dict(before=False, a0=True, a1=True, between=False, b0=True, b1=True)
    assert tr[idx['between']]['final'] == frozenset(['before', 'between', 'b0', 'b1'])
    assert tr[idx['before exit']]['final'] == frozenset(['before', 'between']) and tr[idx['before exit']]['pending'] == ('a0', 'a1', 'b0', 'b1')
    assert [t['flush'] for t in tr if t['flush']] == ['exit']
    q = _find(seqs, 'flush_reduces mid-scope')
    tr = RC.trace(q)
    idx = dict((it[1], i) for i, it in enumerate(q.items) if not isinstance(it, RC.Step) and it[0] == 'check')
    assert tr[idx['flushed']]['final'] == frozenset(q.dests) and tr[idx['flushed']]['applied'] == (0, 1)
    assert tr[idx['recording again']]['final'] == frozenset(['a0', 'a1']) and tr[idx['recording again']]['pending'] == ('b0', 'b1')


def test_coverage_over_the_pinned_lists():
    seqs = RC.all_sequences()
    assert len(set(q.name for q in seqs)) == len(seqs)
    RC.coverage(RC.seen_of(seqs))
    for drop in ('z56 alone', 'table 41', 'table 80', 'same output acc 1/0', 'adjacent vectors of one buffer',
                 'column blocks of one matrix', 'vector inside the span of a pitched block',
                 'mixed col_sum acc 1/0 two-stage then direct, second defer=False',
                 'mixed channel_sum acc 1/1 direct then two-stage, second defer=True', 'outer scope, two inner blocks',
                 'flush_reduces mid-scope', 'scope on a side stream', 'gemm_h destinations'):
        rest = [q for q in seqs if q.name != drop]
        assert len(rest) == len(seqs) - 1
        with pytest.raises(AssertionError, match='no longer reach'):
            RC.coverage(RC.seen_of(rest))
    for cls in ('z sweep', 'table', 'clash', 'mixed', 'scope', 'gemm_h'):
        with pytest.raises(AssertionError, match='no longer reach'):
            RC.coverage(RC.seen_of([q for q in seqs if q.cls != cls]))


def test_exact_pass_keeps_every_sum_exact_and_nonzero():
    for q in RC.all_sequences():
        inputs, starts = RC.make_inputs(q, RC.EXACT)
        for i, s in q.steps():
            assert 9 * RC.red_len(s) < 2 ** 24
            v = RC.value(s, inputs[i], torch.float64)
            assert bool((v > 0).all()) and bool((v == v.round()).all())
        for n, v in starts.items():
            assert bool(torch.isnan(v).all()) if not q.first_acc(n) else bool(((v != 0) & (v == v.round())).all())
        ref = RC.reference(q, inputs, starts)
        assert all(float(v.abs().max()) < 2 ** 24 for v in ref.values())


# ---------------------------------------------------------------------------------------------------------------------
# the Python scope state machine, on a recorder in place of the library
# ---------------------------------------------------------------------------------------------------------------------
class Recorder(object):
    """stands where ``kernels.lib`` stands: every entry point answers 0 (AG_OK) - or what `answers` says - and is written down"""

    def __init__(self, **answers):
        self.calls, self.answers = [], answers

    def __getattr__(self, name):
        def f(*a):
            self.calls.append((name, a))
            return self.answers.get(name, 0)
        return f

    def modes(self):
        """the state machine's calls in order: an int = ag_defer_reduces(mode), 'F' = ag_flush_reduces, a name = a launch"""
        out = []
        for n, a in self.calls:
            if n == 'ag_defer_reduces':
                out.append(a[0])
            elif n == 'ag_flush_reduces':
                out.append('F')
            elif n in ('ag_gemm', 'ag_col_sum', 'ag_gemm_h', 'ag_channel_sum'):
                out.append(n)
        return out


REST = dict(keep=None, outer=False, depth=0)


@pytest.fixture
def rec(monkeypatch):
    import audiogan_amd.kernels as K
    assert K._DEFER == REST
    r = Recorder(ag_gemm_ws_numel=4096, ag_gemm_h_ws_numel=4096)
    monkeypatch.setattr(K, 'lib', r)
    monkeypatch.setattr(K, '_stream', lambda: None)
    monkeypatch.setattr(K, '_chk', lambda *a, **k: None)
    yield K, r
    assert K._DEFER == REST, 'a test left the deferral state open'


def test_scope_roles(rec):
    K, r = rec
    with K.deferred_reduces() as own:
        assert own.role == 'owner' and K.reduces_recording() and not K.reduces_outer()
        with K.deferred_reduces() as inner:                 # an inner block of a plain owner: no mode change, no flush
            assert inner.role == 'inner' and K._DEFER['depth'] == 1
        assert K._DEFER['depth'] == 0 and K.reduces_recording()
    assert r.modes() == [1, 'F', 1, 0] and K._DEFER == REST

    del r.calls[:]
    with K.deferred_reduces(outer=True) as own:
        assert own.role == 'owner' and not K.reduces_recording() and K.reduces_outer()      # paused at once
        with K.deferred_reduces(outer=True) as nest:        # a network scope inside another: the outermost one rules
            assert nest.role == 'nested' and not K.reduces_recording()
            with K.deferred_reduces() as a:                 # resume on the first entry ...
                assert a.role == 'inner' and K.reduces_recording()
                with K.deferred_reduces() as b:
                    assert b.role == 'inner' and K._DEFER['depth'] == 2
                assert K.reduces_recording()
            assert not K.reduces_recording()                # ... pause on the last exit, no flush
        assert K._DEFER['keep'] is not None
        with K.deferred_reduces():
            pass
    assert r.modes() == [1, 2, 3, 2, 3, 2, 'F', 1, 0] and K._DEFER == REST


def test_scope_error_paths(rec):
    K, r = rec
    with pytest.raises(KeyError):
        with K.deferred_reduces():
            K._bind_ws(8, 'cpu')
            raise KeyError('boom')
    assert r.modes() == [1, 1, 0] and K._DEFER == REST       # no flush; drop what was recorded, then off

    del r.calls[:]
    with pytest.raises(KeyError):
        with K.deferred_reduces(outer=True):
            with K.deferred_reduces():
                raise KeyError('boom')
    assert r.modes() == [1, 2, 3, 2, 1, 0] and K._DEFER == REST     # the inner block pauses again on its way out

    del r.calls[:]
    r.answers['ag_flush_reduces'] = -2                        # the flush itself fails: the state still comes to rest
    with pytest.raises(RuntimeError):
        with K.deferred_reduces():
            pass
    assert r.modes() == [1, 'F', 1, 0] and K._DEFER == REST
    r.answers.pop('ag_flush_reduces')

    del r.calls[:]
    K.flush_reduces()                                         # no scope open: nothing
    assert r.calls == []
    with K.deferred_reduces():
        K.flush_reduces()
        assert K.reduces_recording()
    assert r.modes() == [1, 'F', 'F', 1, 0]


def test_immediate_and_hold(rec):
    K, r = rec
    A, B, Cm = torch.zeros(1024, 8), torch.zeros(1024, 8), torch.zeros(8, 8)
    X, out = torch.zeros(32, 8), torch.zeros(8)
    A16, B16 = A.bfloat16(), B.bfloat16()

    def launches():
        K.gemm(A, B, Cm, ta=True, beta=1.0)                   # defer=False: complete on return
        K.gemm(A, B, Cm, ta=True, beta=1.0, defer=True)
        K.col_sum(X, out, defer=False)
        K.col_sum(X, out)
        K.gemm_h(A16, B16, C=Cm, ta=True, beta=1.0)
        K.gemm_h(A16, B16, C=Cm, ta=True, beta=1.0, defer=True)
        with K._immediate():
            K.channel_sum(torch.zeros(2, 8, 4), out)
    plain = ['ag_gemm', 'ag_gemm', 'ag_col_sum', 'ag_col_sum', 'ag_gemm_h', 'ag_gemm_h', 'ag_channel_sum']
    launches()                                                # outside any scope: nothing
    assert r.modes() == plain
    del r.calls[:]
    with K.deferred_reduces():                                # recording: 2 ... 3 around every call that must be complete
        launches()
    assert r.modes() == [1, 2, 'ag_gemm', 3, 'ag_gemm', 2, 'ag_col_sum', 3, 'ag_col_sum', 2, 'ag_gemm_h', 3, 'ag_gemm_h',
                         2, 'ag_channel_sum', 3, 'F', 1, 0]
    del r.calls[:]
    with K.deferred_reduces(outer=True):                      # a paused outer scope: nothing
        launches()
    assert r.modes() == [1, 2] + plain + ['F', 1, 0]
    del r.calls[:]
    r.answers['ag_gemm_ws_numel'] = 0                         # a product that is not split needs no hold
    with K.deferred_reduces():
        K.gemm(A, B, Cm, ta=True)
    assert r.modes() == [1, 'ag_gemm', 'F', 1, 0]
    del r.calls[:]
    r.answers['ag_gemm_ws_numel'] = 4096
    r.answers['ag_gemm'] = -1                                 # the call fails inside a hold: recording resumes all the same
    with pytest.raises(ValueError):
        with K.deferred_reduces():
            K.gemm(A, B, Cm, ta=True)
    assert r.modes() == [1, 2, 'ag_gemm', 3, 1, 0]


def test_bound_workspaces_are_kept_until_the_owner_exits(rec):
    K, r = rec
    assert K._bind_ws(0, 'cpu') is None and r.calls[-1][0] == 'ag_bind_workspace' and r.calls[-1][1][1] == 0
    ws = K._bind_ws(16, 'cpu')
    assert ws.numel() == 16 and r.calls[-1][1][1] == 16 and K._DEFER['keep'] is None          # no scope: nothing kept
    with K.deferred_reduces(outer=True):
        a = K._bind_ws(16, 'cpu')
        with K.deferred_reduces():
            b = K._bind_ws(32, 'cpu')
            K._bind_ws(0, 'cpu')
        assert [t.data_ptr() for t in K._DEFER['keep']] == [a.data_ptr(), b.data_ptr()]        # an inner exit drops nothing
        K.flush_reduces()
        c = K._bind_ws(8, 'cpu')
        assert len(K._DEFER['keep']) == 3 and K._DEFER['keep'][2] is c
    assert K._DEFER == REST
    X, out = torch.zeros(32, 8), torch.zeros(8)
    with K.deferred_reduces():
        K.col_sum(X, out)
        K.col_sum(torch.zeros(8, 8), out)                     # the direct form binds no workspace
        assert [t.numel() for t in K._DEFER['keep']] == [64 * 8]
    assert K._DEFER == REST


# ---------------------------------------------------------------------------------------------------------------------
# the runner and the references, on the CPU kernel model
# ---------------------------------------------------------------------------------------------------------------------
def _host_handful():
    seqs = RC.all_sequences()
    names = ('z9 alone', 'z25 last of five', 'table 41', 'same output acc 1/0', 'column blocks of one matrix',
             'adjacent vectors of one buffer', 'vector inside the span of a pitched block',
             'mixed col_sum acc 1/0 two-stage then direct, second defer=False',
             'mixed gemm acc 1/1 direct then two-stage, second defer=True', 'outer scope, two inner blocks',
             'flush_reduces mid-scope', 'scope on a side stream')
    return [_find(seqs, n) for n in names]


def test_sequences_on_the_cpu_model(monkeypatch):
    import audiogan_amd.kernels as K
    KM.install(monkeypatch)
    worst = {}
    for q in _host_handful():
        RC.check_seq(K, q, 'cpu', worst=worst, pending=False)
    assert worst and max(worst.values()) <= RC.MARGIN


def test_the_checker_rejects_wrong_reductions(monkeypatch):
    import audiogan_amd.kernels as K
    KM.install(monkeypatch)
    q = _find(RC.all_sequences(), 'z9 alone')

    def drops_last_row(X, out, accumulate=True, defer=True):
        KM.col_sum(X[:-1], out, accumulate, defer)

    def ignores_accumulate(X, out, accumulate=True, defer=True):
        KM.col_sum(X, out, False, defer)

    def writes_one_too_many(X, out, accumulate=True, defer=True):
        KM.col_sum(X, out, accumulate, defer)
        out.as_strided((1,), (1,), out.storage_offset() + out.numel()).fill_(1.0)

    for bad in (drops_last_row, ignores_accumulate, writes_one_too_many):
        monkeypatch.setattr(K, 'col_sum', bad)
        with pytest.raises(AssertionError):
            RC.check_seq(K, q, 'cpu', pending=False)
