"""Shared pieces of the stacked-front tests (test_front_stack.py on the CPU, test_gpu_front_stack.py on the GPU)  --  TEST
INFRASTRUCTURE, no test functions, imports no GPU code.

  ref_stack_front()     float64 (or, for the floor, fp32) statement of a Generator front with nl LSTMCell layers, written
                        directly in torch: layer 0 takes [x_{t-1}, zc_t], layer l takes h_{l-1,t}, x_t = tanh(proj h_top),
                        s_t = stop h_top; effective weights g v / ||v||; loss and gradients as recurrent_cases.ref_front.
  stack_fwd_model() / stack_gen_model()   torch models of the CONTRACT of ag_gfront_stack_fwd (include/audiogan_hip.h) in its
                        two modes, with the argument lists of K.gfront_stack_fwd_persist / K.gfront_stack_gen_persist: what the
                        host routing runs on where there is no GPU, and (``mutate``) the wrong launches the checkers must reject.
  CASES / REFUSED       the case table, each case with its reason.
  run_stack_front() / check_stack()   one forward + backward through recurrent.GFrontFn with the frames inside guard floats,
                        and the assertions: the bound rule of tests/recurrent_cases.py (margin * floor, floor = the fp32 run of
                        the reference against its float64 run, never above the ceilings), every output of every case.
"""
import torch

from tests import recurrent_cases as RC
from tests.recurrent_cases import FRONT_FZ, Framed, bound, err_of, margin_of, same_bits      # noqa: F401  (re-exported)

GEN_LAG = 1      # csrc/front_parts.h: the exit test before frame t + 1 reads the decisions of frame t - GEN_LAG

# (nl, S, fs, B, T): every one takes the stacked launch on 256 CUs (asserted with ag_gfront_stack_ok by the tests)
CASES = [dict(id=i, nl=nl, S=S, fs=fs, B=B, T=T, why=why) for i, (nl, S, fs, B, T, why) in enumerate([
    (2, 128, 24, 33, 5, 'two row tiles, a tile of one clip, fs % 16 == 8, both parities'),
    (3, 128, 64, 64, 2, 'fs at the panel width, a middle layer'),
    (2, 128, 8, 1, 1, 'no recurrent term'),
    (2, 128, 8, 1, 3, 'smallest everything'),
    (8, 128, 40, 31, 12, 'deepest chain'),
    (8, 128, 64, 64, 3, '256 workgroups, the full chip'),
    (2, 128, 64, 40, 33, 'long flag sequence'),
    (2, 1024, 200, 32, 3, "the reference's defaults, 256 workgroups"),
    (2, 1024, 256, 7, 2, 'unmasked panel, a partial tile'),
])]
# (nl, S, fs, B): refused by ag_gfront_stack_ok on 256 CUs, these keep the per-frame path
REFUSED = [(2, 1024, 200, 33), (3, 1024, 200, 32), (9, 128, 8, 1), (2, 512, 200, 32), (2, 128, 72, 8),
           (1, 1024, 200, 32), (1, 128, 64, 4), (1, 128, 8, 1)]
N_CU = 256

# (output) -> a margin above 16, at most RC.MARGIN_MAX, each with its reason; measured ratios: profiles/front_stack_fuzz.txt
STACK_MARGINS = {
    # The case of recurrent_cases.MARGINS[('front_lstm_frames', 'dstop.w_g')] again.  The g-gradient of the stop head's weight
    # is ONE number, v . dW_s / ||v||, formed by weight_norm_bwd_kernel as one S-term dot product (code this launch does not
    # touch).  In the case (8, 128, 64, 64, 3) its terms cancel 88-fold (sum |v_j dW_j| / |sum v_j dW_j|, from the float64
    # reference; 4 to 37 in the other cases), so its fp32 error is of the size 88 * 2^-24 = 5.2e-6 of the result whatever the
    # order of summation, while the floor of a one-element tensor is a single draw of that error (1.9e-7 here).  Measured on
    # the MI355X: 7.0e-6, 37 floors.
    'dstop.w_g': 64.0,
}

MUTANTS = ('proj_from_l0', 'lower_prev', 'no_upper_bias', 'stop_prev')


def case_name(case):
    return 'nl%d-S%d-fs%d-B%d-T%d' % (case['nl'], case['S'], case['fs'], case['B'], case['T'])


def param_names(nl):
    """the WNGroup's order: per layer w_ih, w_hh, b_ih, b_hh, then proj.w, proj.b, stop.w, stop.b"""
    return ['l%d.%s' % (l, n) for l in range(nl) for n in RC.FRONT_PARAMS[:4]] + list(RC.FRONT_PARAMS[4:])


def ref_stack_front(nl, zc, vg, gx, gs, dtype=torch.float64, mutate=None):
    """vg: [(v, g)] * (4 nl + 4) in the WNGroup's order.  Returns dict(x [B,T*fs], s [B,T], dzc, grads = [dv0, dg0, dv1, ...])
    in `dtype`.  mutate: a wrong front (one of MUTANTS)"""
    assert mutate is None or mutate in MUTANTS
    T, B, Fz = zc.shape
    zc = zc.to(dtype).clone().requires_grad_(True)
    leaves = [t.to(dtype).clone().requires_grad_(True) for pair in vg for t in pair]
    w = [RC._wn(leaves[2 * i], leaves[2 * i + 1]) for i in range(4 * nl + 4)]
    pw, pb, sw, sb = w[4 * nl:]
    S, fs = w[1].size(1), pw.size(0)
    h = [torch.zeros(B, S, dtype=dtype) for _ in range(nl)]
    c = [torch.zeros(B, S, dtype=dtype) for _ in range(nl)]
    xprev = torch.zeros(B, fs, dtype=dtype)
    xs, ss = [], []
    for t in range(T):
        hold = list(h)
        inp = torch.cat([xprev, zc[t]], 1)
        for l in range(nl):
            w_ih, w_hh, b_ih, b_hh = w[4 * l:4 * l + 4]
            if l > 0:
                inp = hold[l - 1] if (mutate == 'lower_prev' and l == 1) else h[l - 1]
            g = inp @ w_ih.t() + h[l] @ w_hh.t()
            if not (mutate == 'no_upper_bias' and l > 0):
                g = g + b_ih + b_hh
            i, f, gg, o = torch.sigmoid(g[:, :S]), torch.sigmoid(g[:, S:2 * S]), torch.tanh(g[:, 2 * S:3 * S]), \
                torch.sigmoid(g[:, 3 * S:])
            c[l] = f * c[l] + i * gg
            h[l] = o * torch.tanh(c[l])
        xprev = torch.tanh(h[0 if mutate == 'proj_from_l0' else -1] @ pw.t() + pb)
        xs.append(xprev)
        ss.append(((hold[-1] if mutate == 'stop_prev' else h[-1]) @ sw.t() + sb).view(B))
    x, s = torch.cat(xs, 1), torch.stack(ss, 1)
    # (a mutant may leave a parameter out of the graph: its gradient is zero)
    grads = torch.autograd.grad((x * gx.to(dtype)).sum() + (s * gs.to(dtype)).sum(), [zc] + leaves, allow_unused=mutate is not None)
    grads = [torch.zeros_like(t) if q is None else q for q, t in zip(grads, [zc] + leaves)]
    return dict(x=x.detach(), s=s.detach(), dzc=grads[0], grads=list(grads[1:]))


def make_stack_inputs(case):
    nl, S, fs, B, T = case['nl'], case['S'], case['fs'], case['B'], case['T']
    gen = torch.Generator().manual_seed(9000 + case['id'])
    shapes = []
    for l in range(nl):
        shapes += [(4 * S, fs + FRONT_FZ if l == 0 else S), (4 * S, S), (4 * S,), (4 * S,)]
    shapes += [(fs, S), (fs,), (1, S), (1,)]
    vg = []
    for shp in shapes:
        v = torch.randn(shp, generator=gen) / (shp[-1] ** 0.5 if len(shp) > 1 else 4.0)
        # g = ||v|| * (0.75 .. 1.25): not the norm itself, so that dv and dg are both at work
        nrm = v.reshape(shp[0], -1).norm(dim=1) if len(shp) > 1 else v.abs()
        g = (nrm * (0.75 + 0.5 * torch.rand(shp[0], generator=gen))).view([shp[0]] + [1] * (len(shp) - 1))
        vg.append((v, g.clone()))
    zc = torch.randn(T, B, FRONT_FZ, generator=gen)
    gx, gs = torch.randn(B, T * fs, generator=gen), torch.randn(B, T, generator=gen)
    return dict(vg=vg, zc=zc, gx=gx, gs=gs)


# ---------------------------------------------------------------------------------------------------------------------
# torch models of the launch's contract
# ---------------------------------------------------------------------------------------------------------------------
def _model_frames(pre, wx, w_in, whh, bias, wp, bp, mutate, T_run, on_frame):
    """the frame loop both modes share; on_frame(t, act, c, h, x, h_top_prev) -> True to stop before frame t + 1"""
    T, B, S4 = pre.shape
    S, fs, nl = S4 // 4, wp.size(0), len(whh)
    h = [torch.zeros(B, S) for _ in range(nl)]
    c = [torch.zeros(B, S) for _ in range(nl)]
    xp = torch.zeros(B, fs)
    for t in range(T_run):
        hold = list(h)
        act = []
        for l in range(nl):
            if l == 0:
                g = pre[t] + xp @ wx.t() + h[0] @ whh[0].t()
            else:
                below = hold[l - 1] if (mutate == 'lower_prev' and l == 1) else h[l - 1]
                g = below @ w_in[l - 1].t() + h[l] @ whh[l].t()
                if mutate != 'no_upper_bias':
                    g = g + bias[l - 1]
            i, f, gg, o = [fn(q) for fn, q in zip((torch.sigmoid, torch.sigmoid, torch.tanh, torch.sigmoid), g.chunk(4, 1))]
            c[l] = f * c[l] + i * gg
            h[l] = o * torch.tanh(c[l])
            act.append(torch.cat([i, f, gg, o], 1))
        xp = torch.tanh(h[0 if mutate == 'proj_from_l0' else -1] @ wp.t() + bp)
        if on_frame(t, act, c, h, xp, hold[-1]):
            return t + 1
    return T_run


def stack_fwd_model(gates, wx, w_in, whh, bias, wp, bp, hs, cs, x, xt=None, mutate=None):
    """ag_gfront_stack_fwd, gen = 0: gates[0] in = pre / out = activated, gates[l >= 1] out; hs, cs (cs[l][0] = 0 written
    here), x and the optional xt"""
    T, B, _ = gates[0].shape
    fs, nl = wp.size(0), len(gates)
    assert len(whh) == len(hs) == len(cs) == nl and len(w_in) == len(bias) == nl - 1 and nl >= 2
    pre = gates[0].clone()
    for l in range(nl):
        cs[l][0].zero_()

    def on_frame(t, act, c, h, xv, h_top_prev):
        for l in range(nl):
            gates[l][t].copy_(act[l]); cs[l][t + 1].copy_(c[l]); hs[l][t].copy_(h[l])
        x[:, t * fs:(t + 1) * fs] = xv
        if xt is not None:
            xt[t].copy_(xv)
        return False
    _model_frames(pre, wx, w_in, whh, bias, wp, bp, mutate, T, on_frame)


def stack_gen_model(pre, wx, w_in, whh, bias, wp, bp, ws, bs, u, x, s, first, t_run, mutate=None):
    """ag_gfront_stack_fwd, gen = 1: no history; the stop logits from the TOP layer's h, the draws u < sigmoid(s), and the exit
    rule of ag_gfront_fwd: before frame t + 1 the decisions of frame t - GEN_LAG are read, the loop ends iff every clip has
    stopped by then.  x and s are written for the frames run only"""
    T, B, _ = pre.shape
    fs = wp.size(0)
    assert len(w_in) == len(bias) == len(whh) - 1 and len(whh) >= 2
    fst = torch.full((B,), T, dtype=torch.int32)

    def on_frame(t, act, c, h, xv, h_top_prev):
        x[:, t * fs:(t + 1) * fs] = xv
        sv = (h_top_prev if mutate == 'stop_prev' else h[-1]) @ ws.view(-1) + bs
        s[:, t] = sv
        fst[(fst == T) & (u[t] < torch.sigmoid(sv))] = t + 1
        # (the test at the top of frame t + 1: t + 1 > GEN_LAG and every first <= t + 1 - GEN_LAG)
        return t + 1 > GEN_LAG and bool((fst <= t + 1 - GEN_LAG).all())
    ran = _model_frames(pre, wx, w_in, whh, bias, wp, bp, mutate, T, on_frame)
    first.copy_(fst)
    t_run.fill_(ran)


# ---------------------------------------------------------------------------------------------------------------------
# running a front through its autograd block, and the assertions
# ---------------------------------------------------------------------------------------------------------------------
def build_front(case, inp, device):
    from audiogan_amd import ops
    front = ops.GFront(case['fs'], case['nl'], case['S'])
    for v, g in inp['vg']:
        front.group.add(torch.nn.Parameter(v.to(device)), torch.nn.Parameter(g.to(device).clone()))
    return front


def run_stack_front(monkeypatch, case, inp, device, slab=False):
    """forward + backward of one stacked front through recurrent.GFrontFn, the frames written into a NaN-filled
    [B, ctot, T * fs] buffer between guard floats (slab: ctot = 3, channel 0 of a slab, the gradient handed back as a
    row-pitched view).  Returns dict(x, s, dzc, grads, frames_ok) on the CPU"""
    from audiogan_amd import ops, recurrent
    fs, B, T = case['fs'], case['B'], case['T']
    front = build_front(case, inp, device)
    params = list(front.group.params())
    zc = inp['zc'].to(device).clone().requires_grad_(True)      # (a copy: the prepared inputs are shared and stay as they are)
    ctot = 3 if slab else 1
    fr = Framed((B, ctot, T * fs), device)

    def into_frame(front_, B_, n, dev):
        assert (B_, n) == (B, T * fs)
        return fr.t[:, 0, :]
    plain = recurrent._frames_buffer
    monkeypatch.setattr(recurrent, '_frames_buffer', into_frame)
    try:
        x, s = ops.GFrontFn.apply(zc, front, *params)
    finally:
        monkeypatch.setattr(recurrent, '_frames_buffer', plain)
    assert x.data_ptr() == fr.t.data_ptr() and (B == 1 or x.stride(0) == ctot * T * fs)
    gx, gs = inp['gx'].to(device), inp['gs'].to(device)
    if slab:
        gx_wide = torch.zeros(B, 3, T * fs, device=device)
        gx_wide[:, 0] = gx
        x.backward(gx_wide[:, 0], retain_graph=True)
        (s * gs).sum().backward()
    else:
        ((x * gx).sum() + (s * gs).sum()).backward()
    if torch.device(device).type == 'cuda':
        torch.cuda.synchronize()
    ok = fr.intact() and bool(torch.isnan(fr.t[:, 1:]).all())
    if slab:
        ok = ok and not bool(gx_wide[:, 1:].any()) and torch.equal(gx_wide[:, 0], gx)
    cpu = lambda t: t.detach().cpu().clone()      # noqa: E731
    return dict(x=cpu(x), s=cpu(s), dzc=cpu(zc.grad), grads=[cpu(q.grad) for q in params], frames_ok=ok)


def stack_errors(nl, inp, ref, got):
    """{output: error}: x, s, dzc and, per parameter, the .l2 / .elem errors of dv and dg - recurrent_cases.front_errors (with
    its rule for the dv of a bias) applied to each layer's four tensors beside the two heads"""
    e = {}
    for l in range(nl):
        idx = list(range(4 * l, 4 * l + 4)) + list(range(4 * nl, 4 * nl + 4))
        pick = lambda lst: [lst[2 * i + j] for i in idx for j in (0, 1)]      # noqa: E731
        sub = RC.front_errors(dict(vg=[inp['vg'][i] for i in idx]), dict(ref, grads=pick(ref['grads'])),
                              dict(got, grads=pick(got['grads'])))
        for k, v in sub.items():
            layered = any(k.startswith('d' + n + '_') for n in RC.FRONT_PARAMS[:4])
            if layered:
                e['dl%d.%s' % (l, k[1:])] = v
            elif l == 0:
                e[k] = v
    return e


def stack_floor(case, inp, ref):
    """the fp32 run of ref_stack_front against its float64 run"""
    return stack_errors(case['nl'], inp, ref,
                        ref_stack_front(case['nl'], inp['zc'], inp['vg'], inp['gx'], inp['gs'], dtype=torch.float32))


def stack_margin(name):
    m = STACK_MARGINS.get(name.split('.l2')[0].split('.elem')[0], margin_of('front_stack', name))
    assert RC.MARGIN <= m <= RC.MARGIN_MAX
    return m


def check_stack(case, inp, ref, floor, got, again=None, only=None):
    """got: dict(x, s[, dzc, grads, frames_ok]).  only: the outputs to compare (default: all).  Returns {output: error / floor}"""
    tag = case_name(case)
    assert got.get('frames_ok', True), ('guard frame: a store landed outside the frames', tag)
    if only is None:
        errs = stack_errors(case['nl'], inp, ref, got)
    else:
        errs = {k: err_of(got[k], ref[k]) for k in only}
    ratios = {}
    for name, e in errs.items():
        ceil = RC.CEIL_GRAD_L2 if name.endswith('.l2') else RC.CEIL_GRAD_ELEM if name.endswith('.elem') else RC.CEIL
        b = bound(stack_margin(name), floor[name], ceil)
        assert 0 < b <= ceil, ('bound of ' + name, tag, b)
        print('stacked front | %s | %-22s err %.3g floor %.3g bound %.3g' % (tag, name, e, floor[name], b))
        assert e <= b, ('out of bound: ' + name, tag, e, floor[name])
        ratios[name] = e / max(floor[name], RC.FLOOR_MIN)
    if again is not None:
        for k in ('x', 's', 'dzc', 'grads'):
            assert same_bits(got[k], again[k]), ('not reproducible: ' + k, tag)
    return ratios


_PREPARED = {}


def prepared_stack(case):
    """(inputs, float64 reference, floor) of a case, computed once per process and shared; never modified"""
    key = case['id']
    if key not in _PREPARED:
        inp = make_stack_inputs(case)
        ref = ref_stack_front(case['nl'], inp['zc'], inp['vg'], inp['gx'], inp['gs'])
        _PREPARED[key] = (inp, ref, stack_floor(case, inp, ref))
    return _PREPARED[key]
