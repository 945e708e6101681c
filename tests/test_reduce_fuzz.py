"""-m gpu: what happens ACROSS reducing calls inside a ``kernels.deferred_reduces`` scope - the table of 40 recorded second
stages of csrc/api.hip, the one launch that sums them (slab_reduce_multi_kernel), the clash rule, the slab counts of
slab_sum, direct and deferred writes into one destination, the Python scope state machine and the C one - against float64
(tests/reduce_cases.py holds the sequences, the model of the recording rules, the references, the runner and the coverage
assertion; tests/test_reduce_fuzz_host.py pins the model by hand).

Every sequence runs PLAIN (no scope), SCOPED and scoped again, in two passes of values.  Asserted for each:

  every destination of the scoped run is bit for bit the plain run's, the second scoped run bit for bit the first;
  at every named checkpoint (one synchronize each) the destinations that are pending and final are those of model(seq):
    a destination whose writes are all pending still holds its start or its NaN fill bit for bit, and in the integer pass
    every destination holds exactly what the steps that are final give;
  every frame's guard is intact, and so is what a frame holds beside its destinations;
  integer pass: every destination equals the float64 reference exactly;
  randn pass: the bound rule of DESIGN.md section 2 (16 x the error of the same arithmetic in fp32 on the CPU against
    float64, not below 2^-24, never above 1e-4 of the output scale).

f32 precision mode only, plus the bf16-storage products of gemm_h (the bf16 mode of the first stages: tests/test_bf16.py).
Each test prints error / floor for every destination (pytest -s); the largest per kernel label: profiles/reduce_fuzz.txt."""
import pytest
import torch

from tests import reduce_cases as RC

pytestmark = pytest.mark.gpu

WORST = {}
SEEN = []


@pytest.fixture(scope='module')
def K():
    assert torch.cuda.is_available(), 'gpu tests need a GPU'
    import audiogan_amd.kernels as K_
    assert K_.col_sum.__module__ == 'audiogan_amd.kernels', 'real kernels must be in place'
    assert K_.get_precision() == 'f32' and K_._DEFER == dict(keep=None, outer=False, depth=0)
    return K_


def _class(K, seqs):
    worst = {}
    print()
    for q in seqs:
        RC.check_seq(K, q, 'cuda', worst=worst)
        SEEN.append(q.name)
    print('reduce fuzz: largest real-pass error / floor per kernel label')
    for lb in sorted(worst):
        print('  %-40s %6.2f' % (lb, worst[lb]))
        WORST[lb] = max(WORST.get(lb, 0.0), worst[lb])
    assert K._DEFER == dict(keep=None, outer=False, depth=0)
    torch.cuda.synchronize()


def test_constants_restated_in_the_case_module_match_the_library(K):
    assert RC.SMALL_WS == K._SMALL_WS
    q = RC.Seq('forms', 'x')
    for kind in ('gemm', 'gemm_h'):
        for form in ('c', 'pv', 'ps'):
            for two in (True, False):
                s = RC.st_gemm(q, '%s %s %s' % (kind, form, two), form, two, kind=kind)
                p = s.p
                nws = K.lib.ag_gemm_ws_numel(p['M'], p['N'], p['K'], K.ACT_NONE) if kind == 'gemm' else \
                    K.lib.ag_gemm_h_ws_numel(p['M'], p['N'], p['K'], K.ACT_NONE, 0)
                assert nws == (RC.slabs(s) * p['M'] * p['N'] if two else 0), (s, nws)


def test_z_sweep(K):
    _class(K, RC.z_sequences())


def test_table_limit_and_block_routing(K):
    _class(K, RC.table_sequences())


def test_clash_rule(K):
    _class(K, RC.clash_sequences())


def test_mixed_direct_and_deferred_writes(K):
    """a two-stage and a single-writer call into one destination: the library sums the recorded stages before the direct
    write (ag_slab_settle), recording or paused.  Before that rule the two writes landed in the opposite order of their
    calls: acc 1/0 left sum(Y) + sum(X) where the plain route leaves sum(Y)."""
    _class(K, RC.mixed_sequences())


def test_scopes(K):
    _class(K, RC.scope_sequences())


def test_gemm_h_destinations(K):
    _class(K, RC.gemm_h_sequences())


def test_scope_whose_body_raises(K):
    q = [s for s in RC.scope_sequences() if s.name == 'owner scope'][0]
    inputs, starts = RC.make_inputs(q, RC.REAL)
    plain = RC.run(K, q, inputs, starts, 'cuda', False)
    X = torch.ones(32, 8, device='cuda')
    out = torch.full((8,), 5.0, device='cuda')
    with pytest.raises(KeyError):
        with K.deferred_reduces():
            K.col_sum(X, out)
            raise KeyError('boom')
    torch.cuda.synchronize()
    assert K._DEFER == dict(keep=None, outer=False, depth=0)
    assert K.lib.ag_defer_reduces(3) != 0, 'deferral must be off: resume has no scope to resume'
    assert K.lib.ag_flush_reduces(None) == 0
    torch.cuda.synchronize()
    assert bool((out == 5.0).all()), 'the stage recorded by the failed scope was dropped, not summed later'
    again = RC.run(K, q, inputs, starts, 'cuda', False)
    assert again['intact'] and all(RC.same_bits(again['final'][n], plain['final'][n]) for n in q.dests)


def test_c_state_machine(K):
    """argument errors the library returns before any launch"""
    lib = K.lib
    X = torch.ones(32, 8, device='cuda')
    out = torch.full((8,), 5.0, device='cuda')
    stream = K._stream()

    def col_sum():
        ws = torch.empty(64 * 8, device='cuda')
        assert lib.ag_bind_workspace(K._p(ws), ws.numel()) == 0
        assert lib.ag_col_sum(K._p(X), 0, 8, K._p(out), 32, 8, 1, stream) == 0
        return ws

    assert lib.ag_defer_reduces(3) != 0 and b'resume without a scope' in lib.ag_last_error()
    for mode in (-1, 4, 7):
        assert lib.ag_defer_reduces(mode) != 0 and b'mode must be' in lib.ag_last_error()
    try:
        assert lib.ag_defer_reduces(1) == 0
        keep = [col_sum()]
        assert lib.ag_defer_reduces(0) != 0 and b'never flushed' in lib.ag_last_error()      # a stage is pending ...
        torch.cuda.synchronize()
        assert bool((out == 5.0).all())
        assert lib.ag_flush_reduces(stream) == 0                                              # ... and still flushable
        torch.cuda.synchronize()
        assert bool((out == 37.0).all())
        assert lib.ag_defer_reduces(0) == 0
        assert lib.ag_defer_reduces(3) != 0
        assert lib.ag_defer_reduces(1) == 0
        keep.append(col_sum())
        assert lib.ag_defer_reduces(2) == 0 and lib.ag_defer_reduces(3) == 0                  # pause / resume keep it
        assert lib.ag_defer_reduces(1) == 0                                                   # mode 1 drops what was recorded
        assert lib.ag_flush_reduces(stream) == 0 and lib.ag_defer_reduces(0) == 0
        torch.cuda.synchronize()
        assert bool((out == 37.0).all()), 'a dropped stage was summed'
    finally:
        lib.ag_defer_reduces(1)
        lib.ag_defer_reduces(0)
    del keep


def test_coverage_and_report(K):
    """every class this fuzz names is in the lists the tests above walk (each walks ALL of its list)"""
    lists = (RC.z_sequences, RC.table_sequences, RC.clash_sequences, RC.mixed_sequences, RC.scope_sequences, RC.gemm_h_sequences)
    walked = [q for f in lists for q in f()]
    assert [q.name for q in walked] == [q.name for q in RC.all_sequences()]
    RC.coverage(RC.seen_of(walked))
    print('\nreduce fuzz, the classes that ran in this process (%d of %d sequences): largest real-pass error / floor per kernel label'
          % (len(SEEN), len(walked)))
    for lb in sorted(WORST):
        print('  %-40s %6.2f' % (lb, WORST[lb]))
