"""-m gpu: the six statistics a run is judged by - ag_logit_summary, ag_vec_stats, ag_sqnorm_rows and ag_summary_commit of
csrc/pointwise.hip, ag_ltas_power and ag_score_accum of csrc/evalstats.hip - against float64, one test function per family
(tests/stats_cases.py holds the case lists, the restated branches, the float64 references, the runners, the bound rules and
the coverage assertions):

  the logit summary on contiguous, pitched, transposed and column views with every kind of nframes; the vector statistics
  over one to seventeen trips of the stride loop; the squared norms on rows that take the 16-byte and the scalar path inside
  one launch, alone, finished, and handed to the ring; the ring row with all sixteen columns from device words, immediates
  above 2^31, a wrapping cursor and a cursor out of range; the long-term spectrum from one zero-padded frame to three chunks
  with a workspace of the test's own whose unused rows must keep their NaN; the running scores on more than one row per wave
  and more than one trip of the lanes, next to 1e6 and over ten calls.

Every output sits in a sentinel frame that must come back untouched, every input in a frame of NaN; every case runs twice for
identical bits and ag_last_kernel has to name the plan's kernel.  One case per family runs under the bf16 precision mode and on
a side stream: the bits do not move.  Each test prints the largest real-pass error / floor per kernel and output (pytest -s;
profiles/stats_fuzz.txt) and ends in its family's coverage assertion.  tests/test_stats_fuzz_host.py shows on the CPU models
that the checker rejects subtly wrong kernels."""
import pytest
import torch

from tests import stats_cases as SC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def K():
    assert torch.cuda.is_available(), 'gpu tests need a GPU'
    import audiogan_amd.kernels as K_
    return K_


def _family(K, fam):
    worst = {}
    SC.sweep(fam, K, 'cuda', worst=worst)
    print('stats fuzz, %s: largest real-pass error / floor per kernel and output' % fam)
    for key in sorted(worst):
        print('  %-64s %6.2f' % (key, worst[key]))
    SC.mode_invariant(K, fam, 'cuda')
    SC.side_stream(K, fam, 'cuda')
    torch.cuda.synchronize()


def test_constants_restated_in_the_case_module_match_the_library(K):
    assert (SC.COLS, SC.LT_BINS, SC.SCORE_WORDS) == (K.SUMMARY_COLS, K.LTAS_BINS, K.SCORE_WORDS) == (16, 129, 6)
    # LT_CH = 16: 16 frames need no workspace, 17 need two chunks of 129 bins per clip
    assert K.lib.ag_ltas_ws_numel(3, 256 + 15 * 128) == 0 and K.lib.ag_ltas_ws_numel(3, 256 + 16 * 128) == 3 * 2 * 129
    for _, c in SC.ltas_cases():
        assert K.lib.ag_ltas_ws_numel(c.B, c.L) == SC.ltas_plan(c)['ws'], c
        assert K.lt_frames(c.L) == SC.lt_frames(c.L)


def test_logit_summary(K):
    _family(K, 'logit')


def test_vec_stats(K):
    _family(K, 'vec')


def test_sqnorm_rows(K):
    _family(K, 'sqnorm')


def test_summary_commit(K):
    _family(K, 'commit')


def test_summary_commit_replayed_from_a_captured_graph(K):
    """one commit captured on a single stream and replayed five times into a ring of capacity 3: the rows and the sequence
    numbers of five eager calls; a device word that changes between replays is read on every replay"""
    from audiogan_amd import common
    dev = 'cuda'
    part = torch.randn(65, generator=torch.Generator().manual_seed(5)).to(dev)

    def setup():
        ring = SC.FlatFrame((3, SC.COLS), dev, torch.full((3, SC.COLS), SC.RING_FILL, dtype=torch.int32), dtype=torch.int32)
        cur = SC.FlatFrame((2,), dev, torch.tensor([1, 2 ** 31 - 7], dtype=torch.int32), dtype=torch.int32)
        words = torch.tensor([SC._s32(SC.NAN_PAYLOAD), 41, SC._s32(SC.NEG_ZERO)], dtype=torch.int32, device=dev)
        cols = [words[0:1].view(torch.float32), 9, words[1:2], words[2:3].view(torch.float32), None, 2 ** 31 + 5, 1.5] + [None] * 9
        return ring, cur, words, cols
    ring_e, cur_e, words_e, cols_e = setup()
    hist_e = []
    for i in range(5):
        words_e[1] = 41 + i
        K.summary_commit(ring_e.win, cur_e.win, cols_e, part=part, part_col=4)
        hist_e.append(cur_e.window().tolist())
    torch.cuda.synchronize()
    assert hist_e == [[(1 + i + 1) % 3, 2 ** 31 - 7 + i + 1] for i in range(5)]
    ring_g, cur_g, words_g, cols_g = setup()
    torch.cuda.synchronize()
    K.reserve_table_arena()
    mark = K.capture_mark()
    gr = torch.cuda.CUDAGraph()
    common.new_capture()
    try:
        with torch.cuda.graph(gr, capture_error_mode='thread_local'):
            K.summary_commit(ring_g.win, cur_g.win, cols_g, part=part, part_col=4)
    except Exception:
        K.drop_captured_tables(mark)
        raise
    torch.cuda.synchronize()
    # (capturing executes nothing)
    assert bool((ring_g.window() == SC.RING_FILL).all()) and cur_g.window().tolist() == [1, 2 ** 31 - 7]
    hist_g = []
    for i in range(5):
        words_g[1] = 41 + i
        gr.replay()
        hist_g.append(cur_g.window().tolist())
    torch.cuda.synchronize()
    assert hist_g == hist_e
    assert torch.equal(ring_g.window(), ring_e.window()) and torch.equal(cur_g.window(), cur_e.window())
    assert ring_g.window()[:, 2].tolist() == [43, 44, 45] and ring_g.window()[:, 1].tolist() == [2 ** 31 - 5, 2 ** 31 - 4, 2 ** 31 - 3]
    for f in (ring_e, cur_e, ring_g, cur_g):
        assert f.untouched()


def test_ltas_power(K):
    _family(K, 'ltas')


def test_score_accum(K):
    _family(K, 'score')
