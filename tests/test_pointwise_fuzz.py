"""-m gpu: the small kernels every training step runs through - csrc/pointwise.hip, csrc/convlstm.hip and col_sum of
csrc/gemm.hip - against float64, one test function per family (tests/pointwise_cases.py holds the case lists, the restated
dispatch, the float64 references, the runners and the coverage assertions):

  weight norm over a table of tensors; the LSTM / GRU cell kernels and act_bwd2d on column blocks of slabs; the masked BCE
  in its contiguous and its one-launch strided form; act_fwd / act_bwd / axpby / build_zc / critic_batch; grad_norms +
  opt_step on slices of flat buffers; time moments; the transposes and the narrowing conversion; the one-output Linear and
  the column sums in fp32 mode, bf16 mode and with bf16 storage; the Conv2DLSTM pieces and its layer norm.

Passes as in the three other dispatch fuzzes: integer operands wherever the arithmetic allows it - bit for bit -, randn
operands under the bound rule of DESIGN.md section 2 (16 x the error of the fp32 CPU model, never above 1e-4 of the output
scale; bf16 outputs 2^-7), data movement and carried state bit for bit on random floats.  Every output sits in a sentinel
frame that must come back untouched, NaN-filled when the call writes and at a known non-zero start when it accumulates;
fixed-order reductions run twice for identical bits.  None of these kernels reports a name through ag_last_kernel, so the
plans are restated conditions; the numbers the library does offer (ag_rowdot_bwd_ws_numel, wpa_numel / wpb_numel) are asserted
equal.  Each test prints the largest real-pass error / floor per kernel and output (pytest -s; profiles/pointwise_fuzz.txt)
and ends in its family's coverage assertion.  tests/test_pointwise_fuzz_host.py shows on the CPU model that the checker
rejects subtly wrong kernels."""
import pytest
import torch

from tests import pointwise_cases as PC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def K():
    assert torch.cuda.is_available(), 'gpu tests need a GPU'
    import audiogan_amd.kernels as K_
    return K_


def _report(fam, prec, worst):
    print('pointwise fuzz, %s, %s mode: largest real-pass error / floor per kernel and output' % (fam, prec))
    for form in sorted(worst):
        print('  %-64s %6.2f' % (form, worst[form]))


def _family(K, fam, prec='f32'):
    worst = {}
    with K.precision(prec):
        PC.sweep(fam, K, 'cuda', prec=prec, worst=worst)
    _report(fam, prec, worst)
    torch.cuda.synchronize()


def test_constants_restated_in_the_case_module_match_the_library(K):
    assert (PC.ACT_NONE, PC.ACT_LEAKY, PC.ACT_TANH) == (K.ACT_NONE, K.ACT_LEAKY, K.ACT_TANH)
    assert (PC.OPT_RMSPROP, PC.OPT_ADAM) == (K.OPT_RMSPROP, K.OPT_ADAM)
    assert PC.LEAKY_SLOPE == K.LEAKY_SLOPE and PC.REAL['slope'] == K.LEAKY_SLOPE and PC.SMALL_WS == K._SMALL_WS
    for _, c in PC.rd_cases():
        if c.op == 'rowdot':
            assert K.lib.ag_rowdot_bwd_ws_numel(c.M, c.K) == PC.rd_plan(c)['ws'], c
    for e in PC.wn_plan(PC.wn_cases()[0][1])['entries']:
        if e['dim'] == 3:               # the fp32 layouts the case module indexes, followed by their bf16 images
            maps = PC.wn_maps(e)
            assert K.wpa_numel(e['rows'], e['d1'], e['K']) == maps['total_a'] and K.wpb_numel(e['rows'], e['d1'], e['K'], e['s']) == maps['total_b'], e


def test_weight_norm(K):
    _family(K, 'wn')
    PC.mode_invariant(K, 'wn', PC.wn_cases()[0][0], 'cuda')


def test_cells(K):
    _family(K, 'cells')


def test_losses(K):
    _family(K, 'bce')
    for op in ('bce_contig', 'bce_strided'):
        PC.mode_invariant(K, 'bce', lambda c: c.op == op and c.big, 'cuda')


def test_elementwise(K):
    _family(K, 'elem')


def test_optimiser(K):
    _family(K, 'opt')
    PC.mode_invariant(K, 'opt', 'adam all sizes clip gs dev', 'cuda')


def test_time_moments(K):
    _family(K, 'tm')
    PC.mode_invariant(K, 'tm', PC.tm_cases()[5][0], 'cuda')


def test_transposes_and_conversions(K):
    _family(K, 'tr')


@pytest.mark.parametrize('prec', ['f32', 'bf16'])
def test_rowdot_and_col_sum(K, prec):
    _family(K, 'rd', prec)


def test_convlstm_and_layer_norm(K):
    _family(K, 'cl')
