"""Shared pieces of the tests of the stacked front's one-launch backward (test_front_stack_bwd.py on the CPU,
test_gpu_front_stack_bwd.py on the GPU)  --  TEST INFRASTRUCTURE, no test functions, imports no GPU code.

  stack_bwd_chain()     float64 statement of the chain of ag_gfront_stack_bwd (include/audiogan_hip.h), evaluated on a GIVEN
                        history (activated gates, cell states, frames): what a launch's outputs are compared with.
  stack_bwd_model()     torch fp32 model of the launch's CONTRACT with the argument list of K.gfront_stack_bwd_persist: what the
                        host routing runs on where there is no GPU, and (``mutate``) the wrong launches the checkers must reject.
  BWD_CASES / BWD_REFUSED   the case table: stacked_front_cases.CASES (imported, not copied) and one more, each with its reason.
  cpu_history() / run_direct() / check_direct()   a history from the forward model, one direct call of a wrapper with every
                        output NaN-filled between guard floats, and the assertions on it.
"""
import torch

from tests import recurrent_cases as RC
from tests import stacked_front_cases as SC

# (nl, S, fs, B, T): every one takes the one-launch backward on 256 CUs (asserted with ag_gfront_stack_bwd_ok by the tests)
BWD_CASES = list(SC.CASES) + [
    dict(id=len(SC.CASES), nl=3, S=1024, fs=200, B=32, T=2,
         why='a middle layer at S 1024: its second panel lies half in registers, half in LDS; 205 workgroups'),
]
# (nl, S, fs, B): refused by ag_gfront_stack_bwd_ok on 256 CUs, these keep the per-frame chain
BWD_REFUSED = [(2, 1024, 200, 33), (4, 1024, 200, 32), (9, 128, 8, 1), (2, 512, 200, 32), (2, 128, 72, 8),
               (1, 1024, 200, 32), (1, 128, 8, 1)]
N_CU = SC.N_CU

# (output) -> a margin above 16 for the direct launch against the chain, at most RC.MARGIN_MAX, each with its reason.
# None is needed: measured ratios in profiles/front_stack_bwd_fuzz.txt
BWD_MARGINS = {}

MUTANTS = ('input_next', 'ext_l0', 'rec_wih', 'no_dc', 'proj_all', 'row_past_B')


def bwd_margin(name):
    m = BWD_MARGINS.get(name.split('[')[0], RC.MARGIN)
    assert RC.MARGIN <= m <= RC.MARGIN_MAX
    return m


def _cell_bwd(ga, c_prev, c_new, dh, dc_next, S):
    i, f, g, o = ga[:, :S], ga[:, S:2 * S], ga[:, 2 * S:3 * S], ga[:, 3 * S:]
    tc = torch.tanh(c_new)
    dc = dh * o * (1 - tc * tc)
    if dc_next is not None:
        dc = dc + dc_next
    dg = torch.cat([dc * g * i * (1 - i), dc * c_prev * f * (1 - f), dc * i * (1 - g * g), dh * tc * o * (1 - o)], 1)
    return dg, dc * f


def _chain(gates, cs, x, dh_ext, dx_ext, whh, w_in, wx, wp, dtype, mutate=None):
    """frames T-1 .. 0; returns (dgs list of [T,B,4S], dxt [T,B,fs]) in `dtype`"""
    assert mutate is None or mutate in MUTANTS
    nl = len(gates)
    T, B, S4 = gates[0].shape
    S, fs = S4 // 4, wp.size(0)
    c = lambda t: t.to(dtype)      # noqa: E731
    gates, cs, whh, w_in = [c(t) for t in gates], [c(t) for t in cs], [c(t) for t in whh], [c(t) for t in w_in]
    x, wx, wp = c(x), c(wx), c(wp)
    dgs = [torch.zeros(T, B, S4, dtype=dtype) for _ in range(nl)]
    dxt = torch.zeros(T, B, fs, dtype=dtype)
    dcn = [None] * nl
    L = nl - 1
    for t in reversed(range(T)):
        last = t == T - 1
        dx = c(dx_ext[:, t * fs:(t + 1) * fs]) if dx_ext is not None else torch.zeros(B, fs, dtype=dtype)
        if not last:
            dx = dx + dgs[0][t + 1] @ wx
        xt = x[:, t * fs:(t + 1) * fs]
        gx = dx * (1 - xt * xt)
        dxt[t] = gx
        for l in reversed(range(nl)):
            dh = torch.zeros(B, S, dtype=dtype)
            if dh_ext is not None and l == (0 if mutate == 'ext_l0' else L):
                dh = dh + c(dh_ext[t])
            if not last:
                w_rec = w_in[l - 1] if (mutate == 'rec_wih' and l > 0) else whh[l]
                dh = dh + dgs[l][t + 1] @ w_rec
            if l == L or mutate == 'proj_all':
                dh = dh + gx @ wp
            if l < L:
                if mutate == 'input_next':
                    if not last:
                        dh = dh + dgs[l + 1][t + 1] @ w_in[l]
                else:
                    dh = dh + dgs[l + 1][t] @ w_in[l]
            dgs[l][t], dcn[l] = _cell_bwd(gates[l][t], cs[l][t], cs[l][t + 1], dh, None if mutate == 'no_dc' else dcn[l], S)
    return dgs, dxt


def stack_bwd_chain(gates, cs, x, dh_ext, dx_ext, whh, w_in, wx, wp):
    """float64: gx_t = (dx_ext[t] + dg_{0,t+1} W_x)(1 - x_t^2); dh_{L,t} = dh_ext[t] + dg_{L,t+1} W_hh_L + gx_t W_p;
    dh_{l,t} = dg_{l,t+1} W_hh_l + dg_{l+1,t} W_ih_{l+1}; dg_{l,t} = cell backward(dh_{l,t}, dc_{l,t+1})"""
    cpu = lambda t: None if t is None else t.detach().cpu()      # noqa: E731
    return _chain([cpu(t) for t in gates], [cpu(t) for t in cs], cpu(x), cpu(dh_ext), cpu(dx_ext), [cpu(t) for t in whh],
                  [cpu(t) for t in w_in], cpu(wx), cpu(wp), torch.float64)


def stack_bwd_model(gates, cs, x, dh_ext, dx_ext, whh, w_in, wx, wp, dgs, dxt, mutate=None):
    """ag_gfront_stack_bwd in fp32: writes dgs[l] and dxt.  mutate: one of MUTANTS ('row_past_B': a right launch that also
    stores one float behind the last row of dgs[0])"""
    assert len(cs) == len(whh) == len(dgs) == len(gates) and len(w_in) == len(gates) - 1 and len(gates) >= 2
    out, oxt = _chain(list(gates), list(cs), x, dh_ext, dx_ext, list(whh), list(w_in), wx, wp, torch.float32,
                      None if mutate == 'row_past_B' else mutate)
    for l in range(len(gates)):
        dgs[l].copy_(out[l])
    dxt.copy_(oxt)
    if mutate == 'row_past_B':
        d = dgs[0]
        torch.as_strided(d, (1,), (1,), d.storage_offset() + d.numel()).fill_(1.0)


def effective_weights(inp, nl):
    """the materialised weights g v / ||v|| of a case's inputs: (lw [nl][4], pw, pb, sw, sb)"""
    w = [RC._wn(v, g) for v, g in inp['vg']]
    return [w[4 * l:4 * l + 4] for l in range(nl)], w[4 * nl], w[4 * nl + 1], w[4 * nl + 2], w[4 * nl + 3]


def cpu_history(case, inp):
    """gates / hs / cs / x of the forward model (stacked_front_cases.stack_fwd_model) on a case's inputs, and the launch's
    arguments: dict(gates, cs, x, dh_ext, dx_ext, whh, w_in, wx, wp)"""
    nl, S, fs, B, T = case['nl'], case['S'], case['fs'], case['B'], case['T']
    lw, pw, pb, sw, sb = effective_weights(inp, nl)
    wx, wz = lw[0][0][:, :fs], lw[0][0][:, fs:]
    gates = [torch.zeros(T, B, 4 * S) for _ in range(nl)]
    hs = [torch.zeros(T, B, S) for _ in range(nl)]
    cs = [torch.zeros(T + 1, B, S) for _ in range(nl)]
    x = torch.zeros(B, T * fs)
    gates[0].copy_((inp['zc'].reshape(T * B, -1) @ wz.t() + lw[0][2] + lw[0][3]).view(T, B, 4 * S))
    SC.stack_fwd_model(gates, wx, [lw[l][0] for l in range(1, nl)], [lw[l][1] for l in range(nl)],
                       [lw[l][2] + lw[l][3] for l in range(1, nl)], pw, pb, hs, cs, x)
    dh_ext = (inp['gs'].t().reshape(T * B, 1) @ sw.view(1, S)).view(T, B, S)
    return dict(gates=gates, cs=cs, x=x, dh_ext=dh_ext, dx_ext=inp['gx'].clone(), whh=[lw[l][1] for l in range(nl)],
                w_in=[lw[l][0] for l in range(1, nl)], wx=wx, wp=pw)


def run_direct(wrapper, h, device='cpu'):
    """one call of `wrapper` (K.gfront_stack_bwd_persist or a model of it) on the history h, every dgs[l] and dxt NaN-filled
    between guard floats.  Returns dict(dgs, dxt, frames_ok) on the CPU"""
    nl = len(h['gates'])
    T, B, S4 = h['gates'][0].shape
    fs = h['wp'].size(0)
    dgs = [RC.Framed((T, B, S4), device) for _ in range(nl)]
    dxt = RC.Framed((T, B, fs), device)
    wrapper(h['gates'], h['cs'], h['x'], h['dh_ext'], h['dx_ext'], h['whh'], h['w_in'], h['wx'], h['wp'],
            [d.t for d in dgs], dxt.t)
    if torch.device(device).type == 'cuda':
        torch.cuda.synchronize()
    return dict(dgs=[d.value() for d in dgs], dxt=dxt.value(), frames_ok=all(d.intact() for d in dgs) and dxt.intact())


def direct_errors(chain, got):
    """{output: largest error as a fraction of the chain's largest magnitude in that tensor}"""
    dgs, dxt = chain
    e = {'dgs[%d]' % l: RC.err_of(got['dgs'][l], dgs[l]) for l in range(len(dgs))}
    e['dxt'] = RC.err_of(got['dxt'], dxt)
    return e


def check_direct(tag, chain, floor, got, again=None):
    """got / again: run_direct's.  floor: direct_errors of the per-frame path (on the CPU: of the unmutated model) on the same
    history.  The bound: margin * max(floor, 2^-24), never above 1e-4 of the tensor's largest magnitude.  Returns
    {output: error / floor}"""
    assert got['frames_ok'], ('guard frame: a store landed outside an output', tag)
    ratios = {}
    for name, e in direct_errors(chain, got).items():
        b = RC.bound(bwd_margin(name), floor[name], RC.CEIL)
        assert 0 < b <= RC.CEIL, ('bound of ' + name, tag, b)
        print('stacked front bwd | %s | %-8s err %.3g floor %.3g bound %.3g' % (tag, name, e, floor[name], b))
        assert e <= b, ('out of bound: ' + name, tag, e, floor[name])
        ratios[name] = e / max(floor[name], RC.FLOOR_MIN)
    if again is not None:
        assert RC.same_bits(got['dgs'], again['dgs']) and RC.same_bits(got['dxt'], again['dxt']), ('not reproducible', tag)
    return ratios
