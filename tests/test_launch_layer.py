"""The Python launch layer (audiogan_amd.kernels, the fronts' routing in audiogan_amd.recurrent), on the host:

  * which wrappers the Profiler times, and under what - the table below IS the timed set;
  * a timed wrapper with the Profiler off is a straight call;
  * the check table of the recurrent launches: which exception for which fault, naming the tensor;
  * the six ``*_ok`` predicates of the persistent launches: switches, device, the library's rule;
  * every route of the generator fronts issues the K calls it issued before the launch layer was reorganised."""
import json

import pytest
import torch

import audiogan_amd.kernels as K
from tests import launch_recorder as R

# ---- 1. the timed set ------------------------------------------------------------------------------------------------
TIMED_PLAIN = '''channel_sum leaky_bwd col_sum lstm_cell_fwd lstm_cell_bwd weight_norm_fwd weight_norm_bwd bce_logits_fwd
bce_logits_bwd act_fwd act_bwd act_bwd2d axpby grad_norms opt_step gru_cell_fwd gru_cell_bwd rowdot_fwd rowdot_bwd build_zc
critic_batch to_bf16 conv_o1_fwd conv_o1_bwd_data conv_o1_wgrad convlstm_peephole_fwd convlstm_peephole_bwd convlstm_cell_fwd
convlstm_cell_bwd convlstm_out_fwd convlstm_out_bwd layer_norm_hbfw_fwd layer_norm_hbfw_bwd'''.split()
TIMED_NAMED = '''logit_summary sqnorm_rows vec_stats summary_commit ltas_power score_accum melcep_frames dtw_cost dtw_pairs
resample_poly clip_facts clip_gather frame_power activity_segments'''.split()
TIMED_MODEL = dict(
    gemm='_work_gemm', conv_engine='_work_conv', conv_wgrad='_work_wgrad', ema_update='_work_ema', gemm_h='_work_gemm_h',
    skinny_gemm='_work_skinny', lstm_step_fwd='_work_step', _lstm_seq_fwd_range='_work_seq_fwd',
    _lstm_seq_fwd_persist_call='_work_seq_fwd_persist', _lstm_seq_bwd_persist_call='_work_seq_bwd_persist',
    _lstm_seq_bwd_prod='_work_seq_bwd_prod', _lstm_seq_bwd_cell='_work_seq_bwd_cell', _lstm_seq_bwd_step='_work_seq_bwd_step',
    gfront_fwd_persist='_work_gfront', gfront_bwd_persist='_work_gfront_bwd', grufront_fwd_persist='_work_grufront',
    grufront_bwd_persist='_work_grufront_bwd', gfront_stack_fwd_persist='_work_gfront_stack',
    gfront_stack_bwd_persist='_work_gfront_stack_bwd')


def test_the_timed_set_is_the_table():
    assert len(TIMED_PLAIN) == 33 and len(TIMED_NAMED) == 14 and len(TIMED_MODEL) == 19
    want = dict({n: None for n in TIMED_PLAIN}, **{n: K._work_named for n in TIMED_NAMED})
    want.update({n: getattr(K, m) for n, m in TIMED_MODEL.items()})
    assert len(want) == 66
    for name, work in want.items():
        fn = getattr(K, name)
        assert fn.timed_name == name and fn.__name__ == name, name
        assert fn.timed_work is work, (name, fn.timed_work)
    marked = sorted(n for n, v in vars(K).items() if hasattr(v, 'timed_name') or hasattr(v, 'timed_work'))
    assert marked == sorted(want)
    # untimed on purpose: timing them would change the profile bench.py reports
    for name in ('gfront_gen_persist', 'gfront_stack_gen_persist', 'lstm_front_bwd_step', 'bce_logits_fwd_strided',
                 'bce_logits_bwd_strided', 'bct_to_tbc', 'tbc_to_bct', 'time_moments_fwd', 'time_moments_bwd',
                 'lstm_seq_fwd_persist', '_lstm_seq_bwd_range', 'lstm_seq_fwd', 'lstm_seq_bwd'):
        assert name not in marked and callable(getattr(K, name)), name


# ---- 2. profiler off: a straight call ----------------------------------------------------------------------------------
def test_a_timed_wrapper_is_a_straight_call_with_the_profiler_off(monkeypatch):
    class NoCuda(object):
        def __getattr__(self, name):
            raise AssertionError('torch.cuda.%s touched with the Profiler off' % name)
    seen = []

    def stub(a, b=2, *rest, **kw):
        """the stub's words"""
        seen.append((a, b, rest, kw))
        return ('result', a)

    def work(*a, **k):
        raise AssertionError('the work model ran with the Profiler off')
    assert K.Profiler.enabled is False
    monkeypatch.setattr(torch, 'cuda', NoCuda())
    for fn in (K._timed()(stub), K._timed(work)(stub), K._timed(K._work_named, name='other')(stub)):
        del seen[:]
        assert fn(1, 5, 6, key='v') == ('result', 1) and fn(a=3) == ('result', 3)
        assert seen == [(1, 5, (6,), {'key': 'v'}), (3, 2, (), {})]
        assert fn.__doc__ == "the stub's words" and fn.__module__ == 'audiogan_amd.kernels'
    assert fn.timed_name == fn.__name__ == 'other' and fn.timed_work is K._work_named
    assert K.Profiler.records == []


# ---- 3. the check table ------------------------------------------------------------------------------------------------
class OnDevice(object):
    """what the checks read of a tensor, saying it lives on the device (no CUDA tensor can be made on the host)"""

    def __init__(self, t):
        self.t, self.is_cuda = t, True
    dtype = property(lambda self: self.t.dtype)
    shape = property(lambda self: self.t.shape)

    def is_contiguous(self):
        return self.t.is_contiguous()


def _seq_rows(T=3, B=2, H=8, ndir=2, **swap):
    """the rows K._lstm_seq_fwd_range builds for a two-direction pass; ``swap``: name -> the tensor to put there instead"""
    mk = lambda *shp: [OnDevice(torch.zeros(*shp)) for _ in range(ndir)]      # noqa: E731
    lists = dict(pre=mk(T, B, 4 * H), whh=mk(4 * H, H), c_all=mk(T + 1, B, H), hbuf=mk(2, B, H), static=mk(B, 4 * H))
    y = OnDevice(torch.zeros(T, B, ndir * H))
    for name, t in swap.items():
        if name == 'y':
            y = t
        else:
            lists[name[:-3]][int(name[-2])] = t
    return K._per_dir(ndir, (lists['pre'], 'pre', (T, B, 4 * H)), (lists['whh'], 'whh', (4 * H, H)),
                      (lists['c_all'], 'c_all', (T + 1, B, H)), (lists['hbuf'], 'hbuf', (2, B, H)),
                      (lists['static'], 'static', (B, 4 * H))) + [(y, 'y', (T, B, ndir * H), K._F32_OR_BF16)]


def test_check_table_accepts_a_sound_row_set():
    assert K._check_table(_seq_rows()) == {}
    assert K._check_table(_seq_rows(y=OnDevice(torch.zeros(3, 2, 16, dtype=torch.bfloat16)))) == {}
    rows = K._per_dir(2, (None, 'static', (2, 32)), ([OnDevice(torch.zeros(2, 32))] * 2, 'dgsum', (2, 32)))
    assert [r[1] for r in rows] == ['dgsum[0]', 'dgsum[1]'] and K._check_table(rows) == {}


@pytest.mark.parametrize('name,bad,exc', [
    ('whh[1]', torch.zeros(32, 8), RuntimeError),                                        # a CPU tensor
    ('pre[0]', torch.zeros(3, 2, 32), RuntimeError),
    ('c_all[1]', OnDevice(torch.zeros(4, 2, 8, dtype=torch.float64)), TypeError),         # a wrong dtype
    ('hbuf[0]', OnDevice(torch.zeros(2, 2, 8, dtype=torch.bfloat16)), TypeError),         # (bf16 only where the row says so)
    ('y', OnDevice(torch.zeros(3, 2, 16, dtype=torch.float16)), TypeError),
    ('static[1]', OnDevice(torch.zeros(2, 33)), AssertionError),                          # a wrong shape
    ('pre[1]', OnDevice(torch.zeros(2, 3, 32)), AssertionError),
    ('whh[0]', OnDevice(torch.zeros(8, 32).t()), AssertionError),                         # right shape, not contiguous
    ('y', OnDevice(torch.zeros(3, 2, 32)[:, :, ::2]), AssertionError),
])
def test_check_table_raises_by_fault_and_names_the_tensor(name, bad, exc):
    with pytest.raises(exc) as e:
        K._check_table(_seq_rows(**{name: bad}))
    assert name in str(e.value), str(e.value)


def test_check_table_counts_the_directions_and_the_wrappers_use_it():
    with pytest.raises(AssertionError, match='whh'):
        K._per_dir(2, ([OnDevice(torch.zeros(32, 8))], 'whh', (32, 8)))
    z = lambda *shp: [torch.zeros(*shp) for _ in range(2)]      # noqa: E731
    with pytest.raises(RuntimeError, match=r'pre\[0\] must be a CUDA'):
        K._lstm_seq_fwd_range(z(3, 2, 32), z(32, 8), z(4, 2, 8), z(2, 2, 8), torch.zeros(3, 2, 16), None, 0, 3)
    with pytest.raises(RuntimeError, match=r'pre\[0\] must be a CUDA'):
        K.lstm_seq_fwd_persist(z(3, 2, 32), z(32, 8), z(4, 2, 8), torch.zeros(3, 2, 16), None)
    with pytest.raises(RuntimeError, match=r'gates\[0\] must be a CUDA'):
        K._lstm_seq_bwd_range(z(3, 2, 32), z(32, 8), z(4, 2, 8), torch.zeros(3, 2, 16), z(3, 2, 32), z(2, 2, 8), z(2, 2, 8), None, 0, 3)
    with pytest.raises(RuntimeError, match=r'gates\[0\] must be a CUDA'):
        K._lstm_seq_bwd_persist_call(z(3, 2, 32), z(32, 8), z(4, 2, 8), torch.zeros(3, 2, 16), z(3, 2, 32), None)


def test_one_helper_each_for_either_storage_type():
    for t in (torch.zeros(2, 3), torch.zeros(2, 3, dtype=torch.bfloat16)):
        K._chk(OnDevice(t), 't', K._F32_OR_BF16)
    with pytest.raises(TypeError, match='float32 or torch.bfloat16'):
        K._chk(OnDevice(torch.zeros(2, dtype=torch.float16)), 't', K._F32_OR_BF16)
    with pytest.raises(TypeError):
        K._chk(OnDevice(torch.zeros(2, dtype=torch.bfloat16)), 't')
    assert not hasattr(K, '_chk_any') and not hasattr(K, '_mat_any') and not hasattr(K, '_instrument')
    assert not hasattr(K, '_os') and not hasattr(K, '_os1')


# ---- 4. the predicates -------------------------------------------------------------------------------------------------
# name -> (the library's rule, shapes it takes at 256 CUs and shapes it refuses, the switches of the Python side)
PREDICATES = {
    'lstm_persist_ok': ('ag_lstm_persist_ok', [(64, 512, 2), (16, 64, 1)], [(256, 768, 2)], ['PERSIST']),
    'lstm_persist_bwd_ok': ('ag_lstm_persist_bwd_ok', [(64, 512, 2), (16, 64, 1)], [(64, 768, 2)], ['PERSIST']),
    'gfront_persist_ok': ('ag_gfront_persist_ok', [(32, 1024, 200)], [(128, 1024, 200)], ['PERSIST']),
    'gfront_bwd_persist_ok': ('ag_gfront_bwd_persist_ok', [(32, 1024, 200)], [(128, 1024, 200)], ['PERSIST', 'PERSIST_FRONT_BWD']),
    'gfront_stack_ok': ('ag_gfront_stack_ok', [(32, 1024, 200, 2), (8, 128, 64, 3)], [(33, 1024, 200, 2)],
                        ['PERSIST', 'PERSIST_FRONT_STACK']),
    'gfront_stack_bwd_ok': ('ag_gfront_stack_bwd_ok', [(32, 1024, 200, 2)], [(33, 1024, 200, 2)],
                            ['PERSIST', 'PERSIST_FRONT_STACK', 'PERSIST_FRONT_STACK_BWD', 'PERSIST_FRONT_BWD']),
}


@pytest.mark.parametrize('name', sorted(PREDICATES))
def test_predicate_is_switches_device_and_the_librarys_rule(monkeypatch, name):
    entry, takes, refuses, switches = PREDICATES[name]
    asked = []
    monkeypatch.setattr(K, '_n_cu', lambda dev: asked.append(dev) or 256)
    ok, rule = getattr(K, name), getattr(K.lib, entry)
    assert all(getattr(K, s) == [True] for s in switches)
    for dims in takes + refuses:
        says = bool(rule(*dims, 256))
        assert says == (dims in takes), (entry, dims)
        assert ok(*dims, 'cuda') is says and ok(*dims, torch.device('cuda', 0)) is says
        assert ok(*dims, 'cpu') is False and ok(*dims, torch.device('cpu')) is False
        for s in switches:
            sw = getattr(K, s)
            sw[0] = False
            try:
                assert ok(*dims, 'cuda') is False, (name, s)
            finally:
                sw[0] = True
        assert ok(*dims, 'cuda') is says
    assert 'cpu' not in [str(d) for d in asked]         # (a CPU device is answered before the CU count is wanted)
    # the CU count is the patched one, looked up at call time
    monkeypatch.setattr(K, '_n_cu', lambda dev: 1)
    assert ok(*takes[0], 'cuda') is bool(rule(*takes[0], 1)) is False


# ---- 5. same calls, same order -----------------------------------------------------------------------------------------
with open(R.GOLDEN) as _f:
    SEQUENCES = json.load(_f)


def test_every_route_is_on_record():
    assert sorted(SEQUENCES) == sorted('%s/T%d' % (r, T) for r in R.ROUTES for T in R.FRAMES)
    names = lambda key: [c[0] for c in SEQUENCES[key]]      # noqa: E731
    # each record took the route it is named for
    for key, launch in (('lstm1_launch', 'gfront_fwd_persist'), ('lstm1_launch', 'gfront_bwd_persist'),
                        ('lstm2_launch', 'gfront_stack_fwd_persist'), ('lstm2_launch', 'gfront_stack_bwd_persist'),
                        ('gru_launch', 'grufront_fwd_persist'), ('gru_launch', 'grufront_bwd_persist'),
                        ('sample_lstm2_stack', 'gfront_stack_gen_persist'), ('sample_lstm1_launch', 'gfront_gen_persist'),
                        ('sample_gru_launch', 'gfront_gen_persist'), ('lstm1_frames_fs16', 'lstm_front_bwd_step'),
                        ('lstm2_frames_s36', 'lstm_cell_fwd')):
        assert names(key + '/T3').count(launch) == (1 if 'persist' in launch else 3 if launch.endswith('step') else 6), key
        assert launch not in names(key + '/T0'), key
    for key in SEQUENCES:
        if '_frames' in key:
            assert not [n for n in names(key) if n.endswith('_persist')], key


@pytest.mark.parametrize('T', R.FRAMES)
@pytest.mark.parametrize('route', sorted(R.ROUTES))
def test_route_issues_the_recorded_calls_in_the_recorded_order(monkeypatch, route, T):
    got = json.loads(json.dumps(R.record(monkeypatch, route, T)))
    want = SEQUENCES['%s/T%d' % (route, T)]
    assert [c[0] for c in got] == [c[0] for c in want]
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (i, g, w)
