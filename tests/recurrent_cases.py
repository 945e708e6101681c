"""Shared pieces of the recurrent launch fuzz (test_recurrent_fuzz.py on the GPU, test_recurrent_fuzz_host.py against the CPU
model)  --  TEST INFRASTRUCTURE, no test functions, imports no GPU code.

  ref_lstm_layer()      float64 statement of one (bi)directional LSTM layer over a padded batch with its masked steps, written
                        directly in torch double (it does not call tests/kernel_model.py): y, the cells by STEP, the activated
                        gates, dgates as the autograd gradient of sum(y * dy), their time sum.
  ref_front()           float64 (or, for the floor, fp32) statement of a Generator front, LSTM or GRU cell, from the (v, g)
                        parameters of its WNGroup: frames, stop logits and the autograd gradients of every parameter.
  tf_forward() / tf_backward()   teacher-forced ONE-step references for AG_PREC_BF16: the step's inputs are the GPU's own
                        outputs of the step before, both operands of the recurrent product rounded to bf16 (RNE), the rest
                        in float64.  Both sides round identical fp32 values, so the comparison is as tight as in fp32 mode.
  layer_cases() / front_cases()   seeded case tables; the REQUIRED CLASSES are the data right below.  The classes assume 256
                        CUs; the GPU test asserts each case's class with the library's ag_*_ok predicates first.
  run_layer()           one forward + backward through `mod` (audiogan_amd.kernels, or a CPU model of it) with every output
                        NaN-filled in the middle of a larger flat buffer whose guard floats must come back bit-identical.
  check_layer() / check_front() / check_tf()   the assertions.  BOUND RULE: per case and output the
                        FLOOR is the error of the fp32 CPU model against the float64 reference as a fraction of the
                        reference tensor's largest magnitude; the bound is margin * floor, never above the ceilings.
"""
import collections

import torch

from tests import kernel_model as KM

# ---------------------------------------------------------------------------------------------------------------------
# the bound rule
# ---------------------------------------------------------------------------------------------------------------------
# margin * floor: a different summation order (8 K slices through LDS, MFMA chains of 4 / 16 / 32 k) legitimately costs a
# few times the fp32 model's own error.  Measured GPU error / floor per kernel form and output: profiles/recurrent_fuzz.txt
MARGIN = 16.0
MARGIN_MAX = 64.0
# (kernel form, output) -> a margin above 16, at most MARGIN_MAX, each with its reason.  Every other ratio measured on the
# MI355X is below 10 (layer kernels: below 2.5), see profiles/recurrent_fuzz.txt.
MARGINS = {
    # measured 18.7 at S = 1024, fs 200, B 33, T 3 (9.3 on the one-launch form of the same case).  The g-gradient of the stop
    # head's weight is ONE number, v . dW_s / ||v||, which weight_norm_bwd_kernel forms as one 1024-term dot product; at this
    # seed its terms cancel 312-fold (sum |v_j dW_j| / |sum v_j dW_j|), so its fp32 error is of the size 312 * 2^-24 = 2e-5 of
    # the result whatever the order of summation, and it moves with the last bit of h.  The floor of a one-element tensor is a
    # single draw of that error (2e-7 here; the same model gave 1.4e-6 on another host's BLAS), not a bound on it.
    ('front_lstm_frames', 'dstop.w_g'): 64.0,
}
CEIL = 1e-4                  # of the reference tensor's largest magnitude: no bound is ever wider
CEIL_GRAD_L2, CEIL_GRAD_ELEM = 1e-4, 5e-4      # parameter gradients of the fronts (sums over T * B)
BF16_OUT = 2.0 ** -7         # a bf16 output vs RNE(reference), as gemm_cases.check(): one step of the format at the scale,
BF16_FLIPS = 0.02            # ... and fewer than 2 % of the elements off the reference's own rounding
# No fp32 output is closer to a float64 value than the rounding of its own store, 2^-24 of that value.  On a tensor of a few
# elements (a stop head's bias gradient is ONE number) the model's error is a single draw and can fall below that by luck; a
# floor below the format's own rounding would ask more than fp32 can hold.  On the tensors of the layer cases the measured
# floors are 4e-8 .. 6e-7 and this never binds.
FLOOR_MIN = 2.0 ** -24

GUARD = 64                   # guard elements on either side of every output (a multiple of 4 floats: 16-byte alignment)
SENTINEL = -12345.0
NAN = float('nan')


def margin_of(form, output=''):
    m = MARGINS.get((form, output.split('.l2')[0].split('.elem')[0]), MARGIN)
    assert MARGIN <= m <= MARGIN_MAX
    return m


def cdiv(a, b):
    return (a + b - 1) // b


# ---------------------------------------------------------------------------------------------------------------------
# REQUIRED CLASSES (data).  `forms` restates on sizes which launch a case takes on 256 CUs; the GPU test asserts it with
# ag_lstm_persist_ok / ag_lstm_persist_bwd_ok / ag_gfront_persist_ok / ag_gfront_bwd_persist_ok, never with these lines.
# ---------------------------------------------------------------------------------------------------------------------
N_CU = 256
T_POOL = (1, 2, 3, 7, 12)
T_LONG = 33                  # once per kernel family: the exchange parity and a long flag sequence
KINDS = ('none', 'full', 'ragged', 'tail0')          # lengths; each occurs in every class
LAYER_CLASSES = collections.OrderedDict([
    # forward persistent, 32-clip tiles: every H of persist_shape_ok, odd and even H / 64, B as the grid allows
    ('fwd32', dict(H=tuple(range(64, 769, 64)), B=(1, 31, 32, 33, 40, 64), ndir=(1, 2))),
    # forward persistent, 64-clip tiles with a partial last tile: (B, H, ndir, T, lengths)
    ('fwd64', dict(pinned=((150, 256, 2, 7, 'tail0'), (100, 512, 2, 3, 'ragged'), (100, 768, 1, 2, 'full'),
                           (150, 256, 2, 2, 'none')))),
    # backward persistent
    ('bwd', dict(H=(64, 128, 256, 512), B=(1, 15, 16, 17, 40, 70), ndir=(1, 2))),
    # one launch per step: H % 16 != 0 takes the skinny-product backward with its bound workspace
    ('step', dict(H=(8, 24, 40, 96), B=(1, 5, 17, 33, 40, 70), ndir=(1, 2))),
    # persistent forward with per-step backward
    ('mixed', dict(H=(192,), B=(1, 17, 33, 40), ndir=(1, 2))),
])
PERSISTENT_CLASSES = ('fwd32', 'fwd64', 'bwd', 'mixed')      # each runs once more with K.PERSIST[0] = False
COST_MAX = 1.6e8             # T * ndir * B * H * H of one case: the float64 reference stays at a fraction of a second

FRONT_CLASSES = collections.OrderedDict([
    ('s128', dict(S=128, fs=(8, 24, 40, 64), B=(1, 31, 32, 33, 64), T=(1, 2, 5))),
    ('s1024', dict(S=1024, pinned=((200, 33, 3), (256, 64, 2), (8, 1, 2)))),        # (fs, B, T)
])
FRONT_FZ = 24                # noise + embedding columns of the front's input


def fwd_tiling(B, H, ndir, n_cu=N_CU):
    """clip tiles of 32 per workgroup of the persistent forward (1 / 2), 0: the shape takes one launch per step"""
    if H % 64 or H < 64 or H > 768:
        return 0
    for rt in (1, 2):
        if ndir * cdiv(B, 32 * rt) * (H // 8) <= min(n_cu, 256):
            return rt
    return 0


def bwd_persistent(B, H, ndir, n_cu=N_CU):
    return H in (64, 128, 256, 512) and ndir * cdiv(B, 16) * (H // 32) <= min(n_cu, 256)


def front_persistent(B, S, fs, n_cu=N_CU):
    panel = {1024: 256, 128: 64}.get(S, 0)
    ok = 8 <= fs <= panel and fs % 8 == 0
    return (ok and B <= 64 and cdiv(B, 32) * (S // 8) <= n_cu, ok and cdiv(B, 32) * (S // 16 + cdiv(fs, 16)) <= n_cu)


def layer_forms(case, persist=True):
    """(forward form, backward form) of a case: 'fwd_persist<RT>' / 'fwd_step';  'bwd_persist<NU>' / 'bwd_step' (the fused
    step kernel, H % 16 == 0) / 'bwd_skinny' (cell kernel + skinny product)"""
    B, H, ndir = case['B'], case['H'], case['ndir']
    rt = fwd_tiling(B, H, ndir) if persist else 0
    fwd = 'fwd_persist<%d>' % rt if rt else 'fwd_step'
    if persist and bwd_persistent(B, H, ndir):
        return fwd, 'bwd_persist<%d>' % (H // 32)
    return fwd, 'bwd_step' if H % 16 == 0 else 'bwd_skinny'


def bf16_fwd_form(case):
    """the bf16 forward form of the persistent launch is a function of (tiling, H / 64 parity): (RT, PM)"""
    rt = fwd_tiling(case['B'], case['H'], case['ndir'])
    if not rt:
        return None
    return rt, (2 if (case['H'] // 8 // (8 // rt)) % 2 == 0 else 1)


def _mk_case(cls, T, B, H, ndir, kind, ri):
    c = dict(cls=cls, T=T, B=B, H=H, ndir=ndir, kind=kind, static=bool(ri(0, 1)), dgsum=bool(ri(0, 1)))
    fwd, bwd = layer_forms(c)
    # bf16 y / bf16 dy / dg16 exist on the persistent launches only
    c['y16'] = bool(ri(0, 2) == 0) and fwd != 'fwd_step'
    c['dy16'] = bool(ri(0, 2) == 0) and bwd.startswith('bwd_persist')
    c['dg16'] = bool(ri(0, 1)) and bwd.startswith('bwd_persist')
    return c


def _tail_ok(cls, B):
    """can a trailing run of zero-length clips cover a whole tile of this class's launch? (16 clips backward, 32 forward)"""
    return B > 16 if cls == 'bwd' else B > 32


def layer_cases(seed=61):
    """the case table: per class every (H, ndir) and every B (cyclically, as the grid allows), lengths cyclically, T and the
    options drawn; then the pinned cases"""
    gen = torch.Generator().manual_seed(seed)

    def ri(lo, hi):
        return int(torch.randint(lo, hi + 1, (1,), generator=gen))
    out = []
    for cls, spec in LAYER_CLASSES.items():
        if 'pinned' in spec:
            out += [_mk_case(cls, T, B, H, ndir, kind, ri) for B, H, ndir, T, kind in spec['pinned']]
            continue
        combos = [(H, nd) for H in spec['H'] for nd in spec['ndir']]
        for n in range(max(len(combos), 2 * len(spec['B']))):
            H, ndir = combos[n % len(combos)]
            kind = KINDS[(n + n // len(combos)) % 4]
            want = {'fwd32': lambda B: fwd_tiling(B, H, ndir) == 1, 'bwd': lambda B: bwd_persistent(B, H, ndir),
                    'step': lambda B: True, 'mixed': lambda B: fwd_tiling(B, H, ndir) > 0}[cls]
            pool = [B for B in spec['B'] if want(B)]
            if kind == 'tail0':
                tails = [B for B in pool if _tail_ok(cls, B)]
                if tails:
                    pool = tails
                else:
                    kind = 'ragged'         # (H = 768 in both directions holds 32 clips: no whole tile to leave empty)
            pref = spec['B'][n % len(spec['B'])]
            B = pref if pref in pool else pool[n % len(pool)]
            ts = [T for T in T_POOL if T * ndir * B * H * H <= COST_MAX]
            T = ts[ri(0, len(ts) - 1)]
            if cls == 'bwd' and ndir == 1 and n < len(combos):
                T = 2                       # bf16 mode's teacher-forced backward check exists at T = 2 only: every NU
            out.append(_mk_case(cls, T, B, H, ndir, kind, ri))
    # T = 33 once per kernel family: persistent forward + backward, fused per-step forward + backward, skinny backward
    out += [_mk_case('fwd32', T_LONG, 33, 128, 2, 'ragged', ri), _mk_case('step', T_LONG, 17, 96, 2, 'ragged', ri),
            _mk_case('step', T_LONG, 5, 40, 1, 'ragged', ri)]
    # the per-step backward forms at T = 2 (bf16 mode's backward check), whole empty tiles at small T
    out += [_mk_case('step', 2, 40, 24, 2, 'tail0', ri), _mk_case('step', 2, 33, 96, 1, 'ragged', ri),
            _mk_case('mixed', 2, 40, 192, 2, 'tail0', ri), _mk_case('bwd', 3, 17, 64, 2, 'tail0', ri),
            _mk_case('fwd32', 2, 33, 320, 1, 'tail0', ri)]
    for i, c in enumerate(out):
        c['id'] = i
    return out


def front_cases(seed=67):
    gen = torch.Generator().manual_seed(seed)

    def ri(lo, hi):
        return int(torch.randint(lo, hi + 1, (1,), generator=gen))
    out = []
    spec = FRONT_CLASSES['s128']
    pools = {k: [spec[k][j] for j in torch.randperm(len(spec[k]), generator=gen).tolist()] for k in ('fs', 'B', 'T')}
    for i in range(12):          # every fs, B and T at least twice, in seeded combinations
        out.append(dict(cls='s128', S=128, fs=pools['fs'][i % 4], B=pools['B'][i % 5], T=pools['T'][(i + ri(0, 2)) % 3]))
    for j, T in enumerate(spec['T']):
        out[j]['T'] = T
    out += [dict(cls='s1024', S=1024, fs=fs, B=B, T=T) for fs, B, T in FRONT_CLASSES['s1024']['pinned']]
    for i, c in enumerate(out):
        c['id'] = i
    return out


def assert_layer_classes(cases):
    """every required class is in the table (sizes only; the GPU test asserts the launches themselves)"""
    def need(what, it):
        assert any(it), ('layer case table', 'class never met', what)
    for cls, spec in LAYER_CLASSES.items():
        mine = [c for c in cases if c['cls'] == cls]
        for kind in KINDS:
            need((cls, 'lengths', kind), (c['kind'] == kind for c in mine))
        if 'pinned' in spec:
            for B, H, ndir, T, kind in spec['pinned']:
                need((cls, B, H, ndir), ((c['B'], c['H'], c['ndir']) == (B, H, ndir) for c in mine))
            continue
        for H in spec['H']:
            for ndir in spec['ndir']:
                need((cls, 'H', H, 'ndir', ndir), (c['H'] == H and c['ndir'] == ndir for c in mine))
        for B in spec['B']:
            need((cls, 'B', B), (c['B'] == B for c in mine))
    for c in cases:
        fwd, bwd = layer_forms(c)
        want = {'fwd32': fwd == 'fwd_persist<1>', 'fwd64': fwd == 'fwd_persist<2>' and c['B'] % 64 != 0,
                'bwd': bwd.startswith('bwd_persist'), 'step': (fwd, bwd[:5]) == ('fwd_step', 'bwd_s'),
                'mixed': fwd.startswith('fwd_persist') and bwd == 'bwd_step'}[c['cls']]
        assert want, ('case is not of its class', c, fwd, bwd)
        assert c['T'] in T_POOL + (T_LONG,) and c['T'] * c['ndir'] * c['B'] * c['H'] ** 2 <= COST_MAX * 1.3, c
    for T in T_POOL:
        need(('T', T), (c['T'] == T for c in cases))
    for fam in ('fwd_persist', 'bwd_persist', 'fwd_step', 'bwd_step', 'bwd_skinny'):
        need(('T = 33', fam), (c['T'] == T_LONG and fam in ''.join(layer_forms(c)) for c in cases))
    need('skinny backward', (layer_forms(c)[1] == 'bwd_skinny' for c in cases))
    for nu in (2, 4, 8, 16):
        need(('bwd_persist', nu, 'T = 2'), (layer_forms(c)[1] == 'bwd_persist<%d>' % nu and c['T'] == 2 for c in cases))
    for bwd in ('bwd_step', 'bwd_skinny'):
        need((bwd, 'T = 2'), (layer_forms(c)[1] == bwd and c['T'] == 2 for c in cases))
    for form in ((1, 1), (1, 2), (2, 2)):           # (2, 1) cannot occur: see bf16_fwd_form
        need(('bf16 forward form', form), (bf16_fwd_form(c) == form for c in cases))
    for opt in ('static', 'dgsum', 'y16', 'dy16', 'dg16'):
        need((opt, 'on'), (c[opt] for c in cases))
        need((opt, 'off'), (not c[opt] for c in cases))
    need('whole empty 32-clip tile', (c['kind'] == 'tail0' and c['B'] > 32 for c in cases))
    need('whole empty 16-clip tile', (c['kind'] == 'tail0' and layer_forms(c)[1].startswith('bwd_persist') for c in cases))


def assert_front_classes(cases):
    spec = FRONT_CLASSES['s128']
    for key in ('fs', 'B', 'T'):
        for v in spec[key]:
            assert any(c['S'] == 128 and c[key] == v for c in cases), ('front case table', key, v)
    for fs, B, T in FRONT_CLASSES['s1024']['pinned']:
        assert any((c['S'], c['fs'], c['B'], c['T']) == (1024, fs, B, T) for c in cases), (fs, B, T)
    for c in cases:
        assert front_persistent(c['B'], c['S'], c['fs']) == (True, True), c


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------
def make_valid(case, gen):
    T, B, kind = case['T'], case['B'], case['kind']
    if kind == 'none':
        return None
    if kind == 'full':
        return torch.full((B,), T, dtype=torch.int64)
    v = torch.randint(0, T + 1, (B,), generator=gen)
    v[0] = T
    for i, x in enumerate((0, 1, T)):       # ragged including 0, 1 and T wherever the batch has the rows
        if B > i + 1:
            v[i + 1] = x
    if kind == 'tail0':                     # a trailing run of zero-length clips that covers a whole 16- and 32-clip tile
        z0 = 32 * ((B - 1) // 32) if B > 32 else 16 * ((B - 1) // 16)
        assert z0 > 0, case
        v[z0:] = 0
    return v


def make_layer_inputs(case):
    T, B, H, ndir = case['T'], case['B'], case['H'], case['ndir']
    gen = torch.Generator().manual_seed(5000 + case['id'])
    pre = [torch.randn(T, B, 4 * H, generator=gen) for _ in range(ndir)]
    whh = [torch.randn(4 * H, H, generator=gen) / H ** 0.5 for _ in range(ndir)]
    static = [torch.randn(B, 4 * H, generator=gen) * 0.5 for _ in range(ndir)] if case['static'] else None
    dy = torch.randn(T, B, ndir * H, generator=gen)
    if case['dy16']:
        dy = dy.bfloat16().float()          # the values a bf16 dy holds; the reference reads the same ones
    return dict(pre=pre, whh=whh, static=static, dy=dy, valid=make_valid(case, gen))


def live_mask(valid, T, B):
    """[T, B] bool: row b is live at time t iff t < valid[b]"""
    if valid is None:
        return torch.ones(T, B, dtype=torch.bool)
    return torch.arange(T).view(T, 1) < valid.view(1, B)


# ---------------------------------------------------------------------------------------------------------------------
# float64 references
# ---------------------------------------------------------------------------------------------------------------------
def ref_lstm_layer(pre, whh, valid, static, dy):
    """per direction, step k visits time t = k (forward) / T-1-k (reverse); g = pre[t] + static + h W_hh^T (no product at
    k = 0); a live row (t < valid[b]) takes the cell update and its y is h, a padded row carries c and h and its y is 0.
    Returns dict(y [T,B,ndir*H], c_all[d] [T+1,B,H] by STEP, gates[d] [T,B,4H] activated, dgates[d], dgsum[d], live [T,B])"""
    ndir = len(pre)
    T, B, H4 = pre[0].shape
    H = H4 // 4
    live = live_mask(valid, T, B)
    P = [p.double().clone().requires_grad_(True) for p in pre]
    ys, c_all, gates = [], [], []
    for d in range(ndir):
        W = whh[d].double()
        h, c = torch.zeros(B, H, dtype=torch.float64), torch.zeros(B, H, dtype=torch.float64)
        cs, yd, gd = [c], [None] * T, [None] * T
        for k in range(T):
            t = k if d == 0 else T - 1 - k
            g = P[d][t]
            if static is not None:
                g = g + static[d].double()
            if k > 0:
                g = g + h @ W.t()
            i, f, gg, o = torch.sigmoid(g[:, :H]), torch.sigmoid(g[:, H:2 * H]), torch.tanh(g[:, 2 * H:3 * H]), \
                torch.sigmoid(g[:, 3 * H:])
            cn = f * c + i * gg
            hn = o * torch.tanh(cn)
            m = live[t].view(B, 1)
            c, h = torch.where(m, cn, c), torch.where(m, hn, h)
            yd[t] = torch.where(m, hn, torch.zeros_like(hn))
            gd[t] = torch.cat([i, f, gg, o], 1).detach()
            cs.append(c.detach())
        ys.append(torch.stack(yd))
        c_all.append(torch.stack(cs))
        gates.append(torch.stack(gd))
    y = torch.cat(ys, 2)
    dg = torch.autograd.grad((y * dy.double()).sum(), P)
    return dict(y=y.detach(), c_all=c_all, gates=gates, dgates=list(dg), dgsum=[g.sum(0) for g in dg], live=live)


def _wn(v, g):
    rows = v.size(0)
    v2 = v.reshape(rows, -1)
    return (v2 * (g.reshape(rows, 1) / v2.norm(dim=1, keepdim=True))).view(v.shape)


def ref_front(cell, zc, vg, gx, gs, dtype=torch.float64, mutate=None):
    """frame t: input [x_{t-1}, zc_t] with x_{-1} = 0; LSTMCell / GRUCell (torch's algebra: n = tanh(i_n + r * (h_n + b_hn)));
    x_t = tanh(proj h_t), s_t = stop h_t; effective weights g * v / ||v||_row; loss = sum(x * gx) + sum(s * gs).
    vg: [(v, g)] * 8 in the WNGroup's order (w_ih, w_hh, b_ih, b_hh, proj.w, proj.b, stop.w, stop.b).
    Returns dict(x [B,T*fs], s [B,T], dzc, grads = [dv0, dg0, dv1, ...]) in `dtype`.  mutate: a wrong front (host test)"""
    T, B, Fz = zc.shape
    zc = zc.to(dtype).clone().requires_grad_(True)
    leaves = [t.to(dtype).clone().requires_grad_(True) for pair in vg for t in pair]
    w_ih, w_hh, b_ih, b_hh, pw, pb, sw, sb = [_wn(leaves[2 * i], leaves[2 * i + 1]) for i in range(8)]
    S, fs = w_hh.size(1), pw.size(0)
    h = torch.zeros(B, S, dtype=dtype)
    c = torch.zeros(B, S, dtype=dtype)
    xprev = torch.zeros(B, fs, dtype=dtype)
    xs, ss = [], []

    def frame(xprev, h, c, t):
        inp = torch.cat([xprev, zc[t]], 1)
        if cell == 'lstm':
            g = inp @ w_ih.t() + b_ih + h @ w_hh.t() + b_hh
            i, f, gg, o = torch.sigmoid(g[:, :S]), torch.sigmoid(g[:, S:2 * S]), torch.tanh(g[:, 2 * S:3 * S]), \
                torch.sigmoid(g[:, 3 * S:])
            c = f * c + i * gg
            hn = o * torch.tanh(c)
        else:
            gi, gh = inp @ w_ih.t() + b_ih, h @ w_hh.t()
            r = torch.sigmoid(gi[:, :S] + gh[:, :S] + b_hh[:S])
            z = torch.sigmoid(gi[:, S:2 * S] + gh[:, S:2 * S] + b_hh[S:2 * S])
            if mutate == 'bhn_outside':
                n = torch.tanh(gi[:, 2 * S:] + r * gh[:, 2 * S:] + b_hh[2 * S:])
            else:
                n = torch.tanh(gi[:, 2 * S:] + r * (gh[:, 2 * S:] + b_hh[2 * S:]))
            hn = (1 - z) * n + z * h
        return hn, c, torch.tanh(hn @ pw.t() + pb)
    for t in range(T):
        hn, cn, x = frame(xprev, h, c, t)
        if mutate == 'xprev_is_x0' and t == 0:
            hn, cn, x = frame(x, h, c, t)
        ss.append(((h if mutate == 'stop_prev' else hn) @ sw.t() + sb).view(B))
        h, c, xprev = hn, cn, x
        xs.append(x)
    x, s = torch.cat(xs, 1), torch.stack(ss, 1)
    grads = torch.autograd.grad((x * gx.to(dtype)).sum() + (s * gs.to(dtype)).sum(), [zc] + leaves)
    return dict(x=x.detach(), s=s.detach(), dzc=grads[0], grads=list(grads[1:]))


def make_front_inputs(case, cell):
    S, fs, B, T = case['S'], case['fs'], case['B'], case['T']
    ng = 3 if cell == 'gru' else 4
    gen = torch.Generator().manual_seed(7000 + case['id'] + (500 if cell == 'gru' else 0))
    shapes = [(ng * S, fs + FRONT_FZ), (ng * S, S), (ng * S,), (ng * S,), (fs, S), (fs,), (1, S), (1,)]
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
# outputs inside guard frames
# ---------------------------------------------------------------------------------------------------------------------
class Framed(object):
    """a tensor of `shape` in the middle of a larger flat buffer: GUARD sentinel elements on either side, the window filled
    with `fill` (NaN: an element the kernel never writes stays visible)"""

    def __init__(self, shape, device, dtype=torch.float32, fill=NAN):
        n = 1
        for s in shape:
            n *= s
        self.n = n
        self.flat = torch.full((n + 2 * GUARD,), SENTINEL, dtype=dtype, device=device)
        self.t = self.flat[GUARD:GUARD + n].view(shape)
        if torch.is_tensor(fill):
            self.t.copy_(fill)
        else:
            self.t.fill_(fill)
        self.before = self._guards()

    def _guards(self):
        f = self.flat.detach().cpu()
        bits = torch.int32 if f.dtype == torch.float32 else torch.int16
        return torch.cat([f[:GUARD], f[GUARD + self.n:]]).clone().view(bits)

    def intact(self):
        return torch.equal(self._guards(), self.before)

    def value(self):
        return self.t.detach().cpu().clone()


def same_bits(a, b):
    if a is None or b is None:
        return a is None and b is None
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(same_bits(x, y) for x, y in zip(a, b))
    bits = torch.int32 if a.dtype == torch.float32 else torch.int16
    return a.shape == b.shape and torch.equal(a.contiguous().view(bits), b.contiguous().view(bits))


def run_layer(mod, case, inp, device, options=True):
    """one forward + backward of a layer through `mod` as recurrent.LSTMSeqFn drives it.  options=False: fp32 y / dy and no
    dg16 whatever the case says (forms without them; bf16 mode's teacher-forced checks read an fp32 y).
    Returns dict(y, gates, c_all, dgates, dgsum, dg16, frames_ok) on the CPU"""
    T, B, H, ndir = case['T'], case['B'], case['H'], case['ndir']
    y16, dy16, dg16 = [case[k] and options for k in ('y16', 'dy16', 'dg16')]
    fr = []

    def framed(shape, dtype=torch.float32, fill=NAN):
        fr.append(Framed(shape, device, dtype, fill))
        return fr[-1].t
    p = [framed((T, B, 4 * H), fill=t) for t in inp['pre']]
    w = [t.to(device) for t in inp['whh']]
    st = [t.to(device) for t in inp['static']] if inp['static'] is not None else None
    v = inp['valid'].to(device) if inp['valid'] is not None else None
    c = [framed((T + 1, B, H)) for _ in range(ndir)]
    if not mod.lstm_persist_ok(B, H, ndir, device):
        for t in c:
            t[0].zero_()                    # (the persistent launch writes c_0 = 0 itself)
    y = framed((T, B, ndir * H), torch.bfloat16 if y16 else torch.float32)
    scratch = lambda: [torch.full((2, B, H), NAN, device=device) for _ in range(ndir)]      # noqa: E731
    mod.lstm_seq_fwd(p, w, c, scratch(), y, v, static=st)
    dy = inp['dy'].to(device)
    if dy16:
        dy = dy.bfloat16()
    dg = [framed((T, B, 4 * H)) for _ in range(ndir)]
    dgs = [framed((B, 4 * H)) for _ in range(ndir)] if case['dgsum'] else None
    kw, d16 = {}, None
    if dg16:                                # two column blocks of ONE [T, B, ndir * 4H] bf16 tensor
        d16 = framed((T, B, ndir * 4 * H), torch.bfloat16)
        kw['dg16'] = [d16[:, :, d * 4 * H:(d + 1) * 4 * H] for d in range(ndir)]
    have = mod.lstm_seq_bwd(p, w, c, dy, dg, scratch(), scratch(), v, dgsum=dgs, **kw)
    if dgs is not None and not have:        # the per-step kernels leave the time sum to a pass over dgates
        for d in range(ndir):
            mod.col_sum(dg[d].view(T, B * 4 * H), dgs[d].view(-1), accumulate=False, defer=False)
    cpu = lambda ts: [t.detach().cpu().clone() for t in ts] if ts is not None else None      # noqa: E731
    return dict(y=y.detach().cpu().clone(), gates=cpu(p), c_all=cpu(c), dgates=cpu(dg), dgsum=cpu(dgs),
                dg16=d16.detach().cpu().clone() if d16 is not None else None, frames_ok=all(f.intact() for f in fr))


class Model(object):
    """tests/kernel_model.py behind the interface run_layer() drives: the fp32 CPU model whose error is the FLOOR.  A bf16 y /
    dg16 is the RNE image of the fp32 result; the time sum is a pass over dgates"""
    lstm_seq_fwd_fn = staticmethod(KM.lstm_seq_fwd)
    lstm_seq_bwd_fn = staticmethod(KM.lstm_seq_bwd)
    col_sum = staticmethod(KM.col_sum)

    def lstm_persist_ok(self, B, H, ndir, dev):
        return False

    def lstm_seq_fwd(self, pre, whh, c_all, hbuf, y, valid, static=None):
        y32 = y if y.dtype == torch.float32 else torch.full(tuple(y.shape), NAN)
        self.lstm_seq_fwd_fn(pre, whh, c_all, hbuf, y32, valid, static=static)
        if y32 is not y:
            y.copy_(y32)

    def lstm_seq_bwd(self, gates, whh, c_all, dy, dgates, dhbuf, dcbuf, valid, dgsum=None, dg16=None):
        self.lstm_seq_bwd_fn(gates, whh, c_all, dy.float(), dgates, dhbuf, dcbuf, valid)
        for d in range(len(gates) if dg16 is not None else 0):
            dg16[d].copy_(dgates[d])
        return False


def err_of(got, ref, mask=None):
    """largest |got - ref| over the compared elements as a fraction of the reference tensor's largest magnitude there"""
    d = (got.double() - ref).abs()
    r = ref.abs()
    if mask is not None:
        m = mask.expand_as(d)
        d, r = d[m], r[m]
    if d.numel() == 0:
        return 0.0
    scale = float(r.max())
    e = float(d.max())
    if e != e:
        return float('inf')
    return e / scale if scale > 0 else (0.0 if e == 0 else float('inf'))


LAYER_OUTPUTS = ('y', 'c_all', 'gates', 'dgates', 'dgsum')


def layer_errors(case, ref, got):
    """{output: error as a fraction of the scale}, the worst direction; y (fp32 only) and dgates over ALL elements, c_all over
    all steps and rows (a padded row carries), the activated gates at live (t, b) only"""
    T, B, H, ndir = case['T'], case['B'], case['H'], case['ndir']
    live3 = ref['live'].view(T, B, 1)
    e = {}
    if got['y'].dtype == torch.float32:
        e['y'] = err_of(got['y'], ref['y'])
    e['c_all'] = max(err_of(got['c_all'][d], ref['c_all'][d]) for d in range(ndir))
    e['gates'] = max(err_of(got['gates'][d], ref['gates'][d], live3) for d in range(ndir))
    e['dgates'] = max(err_of(got['dgates'][d], ref['dgates'][d]) for d in range(ndir))
    if got['dgsum'] is not None:
        e['dgsum'] = max(err_of(got['dgsum'][d], ref['dgsum'][d]) for d in range(ndir))
    return e


def layer_floor(case, inp, ref):
    """the fp32 CPU model's own errors against the float64 reference: what margin * floor starts from"""
    full = dict(case, y16=False, dy16=False, dg16=False, dgsum=True)
    return layer_errors(full, ref, run_layer(Model(), full, inp, 'cpu'))


def bound(margin, floor, ceil=CEIL):
    return min(margin * max(floor, FLOOR_MIN), ceil)


def _check_bf16_image(name, got16, ref, tag):
    want = ref.float().bfloat16().double()
    scale = max(float(ref.abs().max()), 1e-30)
    d = (got16.double() - want).abs()
    assert bool(torch.isfinite(got16.float()).all()), ('not written: ' + name, tag)
    assert float(d.max()) <= BF16_OUT * scale, ('out of bound: ' + name, tag, float(d.max()) / scale)
    assert float((d > 0).double().mean()) < BF16_FLIPS, ('off its rounding: ' + name, tag)


def check_layer(case, ref, floor, got, forms=None, again=None):
    """the assertions on run_layer()'s result; returns {output: error / floor}.  forms: (forward, backward) kernel form, for
    the margins; again: the result of a second identical call"""
    T, B, H, ndir = case['T'], case['B'], case['H'], case['ndir']
    forms = forms or ('model', 'model')
    tag = (case, forms)
    assert got['frames_ok'], ('guard frame: a store landed outside an output', tag)
    live = ref['live']
    pad3 = (~live).view(T, B, 1)
    y = got['y']
    # padded (t, b): y and dgates are EXACTLY 0 (a NaN left there fails this too)
    assert bool((y.float()[pad3.expand_as(y)] == 0).all()), ('padded y is not 0', tag)
    for d in range(ndir):
        dg = got['dgates'][d]
        assert bool((dg[pad3.expand_as(dg)] == 0).all()), ('padded dgates is not 0', tag)
    errs = layer_errors(case, ref, got)
    ratios = {}
    for name in LAYER_OUTPUTS:
        if name not in errs:
            continue
        m = margin_of(forms[0] if name in ('y', 'c_all', 'gates') else forms[1], name)
        b = bound(m, floor[name])
        assert 0 < b <= CEIL, ('bound of ' + name, tag, b)
        assert errs[name] <= b, ('out of bound: ' + name, tag, errs[name], floor[name])
        ratios[name] = errs[name] / max(floor[name], FLOOR_MIN)
    if y.dtype == torch.bfloat16:
        _check_bf16_image('y16', y, ref['y'], tag)
    if got['dg16'] is not None:
        _check_bf16_image('dg16', got['dg16'], torch.cat(ref['dgates'], 2), tag)
        pad16 = pad3.expand_as(got['dg16'])
        assert bool((got['dg16'].float()[pad16] == 0).all()), ('padded dg16 is not 0', tag)
    if again is not None:
        for k in ('y', 'gates', 'c_all', 'dgates', 'dgsum', 'dg16'):
            assert same_bits(got[k], again[k]), ('not reproducible: ' + k, tag)
    return ratios


# ---------------------------------------------------------------------------------------------------------------------
# AG_PREC_BF16: teacher-forced one-step references.  The contract: both operands of the recurrent product rounded to bf16
# with RNE, accumulation and everything else fp32.
# ---------------------------------------------------------------------------------------------------------------------
def rnd(t):
    return t.float().bfloat16().float()


def _cell(g, c_prev, H):
    i, f, gg, o = torch.sigmoid(g[..., :H]), torch.sigmoid(g[..., H:2 * H]), torch.tanh(g[..., 2 * H:3 * H]), \
        torch.sigmoid(g[..., 3 * H:])
    c = f * c_prev + i * gg
    return torch.cat([i, f, gg, o], -1), c, o * torch.tanh(c)


def _step_index(T, d):
    """k(t): the step at which direction d visits time t"""
    t = torch.arange(T)
    return t if d == 0 else T - 1 - t


def tf_forward(case, inp, got, dtype=torch.float64, rounded=True):
    """every step of the forward recomputed from the GPU's own outputs of the step before: h_{k-1} = y[t-1] (forward) /
    y[t+1] (reverse; 0 at a padded step, which is also what a row that has not started yet carries), c_{k-1} = c_all[k].
    Returns per direction (gates, c, h), each [T, B, .] indexed by TIME"""
    T, B, H, ndir = case['T'], case['B'], case['H'], case['ndir']
    out = []
    y = got['y'].float()
    for d in range(ndir):
        yd = y[:, :, d * H:(d + 1) * H]
        hp = torch.zeros(T, B, H)
        if T > 1:
            if d == 0:
                hp[1:] = yd[:-1]
            else:
                hp[:-1] = yd[1:]
        W = inp['whh'][d]
        if rounded:
            hp, W = rnd(hp), rnd(W)
        g = inp['pre'][d].to(dtype) + (hp.to(dtype).view(T * B, H) @ W.to(dtype).t()).view(T, B, 4 * H)
        if inp['static'] is not None:
            g = g + inp['static'][d].to(dtype)
        cp = got['c_all'][d][_step_index(T, d)].to(dtype)
        out.append(_cell(g, cp, H))
    return out


def _cell_bwd(ga, c_prev, c_new, dh, dc_next, H):
    i, f, gg, o = ga[..., :H], ga[..., H:2 * H], ga[..., 2 * H:3 * H], ga[..., 3 * H:]
    tc = torch.tanh(c_new)
    dc = dc_next + dh * o * (1 - tc * tc)
    return torch.cat([dc * gg * i * (1 - i), dc * c_prev * f * (1 - f), dc * i * (1 - gg * gg), dh * tc * o * (1 - o)], -1), dc * f


def tf_backward(case, inp, got, live, dtype=torch.float64, rounded=True):
    """T = 2.  The last step (k = 1) has no recurrent term and its dc is determined by the inputs: compared directly.  Step 0
    from rnd(dgates_1 of the GPU) @ rnd(W_hh) and dc_1 * f_1 (a row padded at step 1 passes 0 on).  The saved gates and cells
    are the GPU's.  Returns per direction dgates [2, B, 4H] by TIME"""
    T, B, H, ndir = case['T'], case['B'], case['H'], case['ndir']
    assert T == 2
    out = []
    dy = inp['dy'].to(dtype)
    for d in range(ndir):
        t1, t0 = (1, 0) if d == 0 else (0, 1)
        ga, c = got['gates'][d].to(dtype), got['c_all'][d].to(dtype)
        zero = torch.zeros(B, H, dtype=dtype)
        m1, m0 = live[t1].view(B, 1), live[t0].view(B, 1)
        dg1, dc1 = _cell_bwd(ga[t1], c[1], c[2], dy[t1, :, d * H:(d + 1) * H], zero, H)
        dg1, dc1 = torch.where(m1, dg1, torch.zeros_like(dg1)), torch.where(m1, dc1, zero)
        A, W = got['dgates'][d][t1], inp['whh'][d]
        if rounded:
            A, W = rnd(A), rnd(W)
        dh0 = A.to(dtype) @ W.to(dtype) + dy[t0, :, d * H:(d + 1) * H]
        dg0, _ = _cell_bwd(ga[t0], c[0], c[1], dh0, dc1, H)
        dg0 = torch.where(m0, dg0, torch.zeros_like(dg0))
        r = torch.zeros(2, B, 4 * H, dtype=dtype)
        r[t1], r[t0] = dg1, dg0
        out.append(r)
    return out


def check_tf(case, inp, got, live, forms):
    """bf16 mode: the GPU's step outputs against the float64 evaluation of the rounded step (floor: the fp32 evaluation of
    the same step), and more than 10 times further from the unrounded step wherever the product is long enough to tell
    (K >= 36, as the GEMM fuzz).  Returns {output: error / floor}"""
    T, B, H, ndir = case['T'], case['B'], case['H'], case['ndir']
    tag = (case, forms, 'bf16')
    live3 = live.view(T, B, 1)
    ref, f32 = tf_forward(case, inp, got), tf_forward(case, inp, got, dtype=torch.float32)
    full = tf_forward(case, inp, got, rounded=False)
    y = got['y']
    ratios = {}

    def one(name, g, r, f, u, m, form, tell):
        e, fl = err_of(g, r, m), err_of(f, r, m)
        b = bound(margin_of(form, name), fl)
        assert e <= b, ('out of bound: ' + name, tag, e, fl)
        ratios[name] = max(ratios.get(name, 0.0), e / max(fl, FLOOR_MIN))
        if tell:
            far = err_of(g, u, m)
            assert far > 10 * e, ('bf16 mode did not round its operands: ' + name, tag, e, far)
    for d in range(ndir):
        # the product exists at k > 0 only: time 1.. (forward) / ..T-2 (reverse), and only rows live there
        mk = torch.zeros_like(live3)
        if T > 1 and d == 0:
            mk[1:] = live3[1:]
        elif T > 1:
            mk[:-1] = live3[1:]             # (reverse: h_{k-1} is not 0 only where the row was live one time step later)
        tell = H >= 36 and bool(mk.any())
        one('gates', got['gates'][d], ref[d][0], f32[d][0], full[d][0], live3, forms[0], False)
        if tell:
            one('gates (k > 0)', got['gates'][d], ref[d][0], f32[d][0], full[d][0], mk, forms[0], True)
        ct = got['c_all'][d][_step_index(T, d) + 1]
        one('c_all', ct, ref[d][1], f32[d][1], full[d][1], live3, forms[0], False)
        one('y', y[:, :, d * H:(d + 1) * H], ref[d][2], f32[d][2], full[d][2], live3, forms[0], False)
    if T == 2:
        rb, fb = tf_backward(case, inp, got, live), tf_backward(case, inp, got, live, dtype=torch.float32)
        ub = tf_backward(case, inp, got, live, rounded=False)
        for d in range(ndir):
            t0 = 0 if d == 0 else 1
            m0 = torch.zeros(2, B, 1, dtype=torch.bool)
            m0[t0] = (live[t0] & live[1 - t0]).view(B, 1)       # the product term reaches rows live at both steps
            one('dgates', got['dgates'][d], rb[d], fb[d], ub[d], None, forms[1], False)
            if 4 * H >= 36 and bool(m0.any()):
                one('dgates (k = 0)', got['dgates'][d], rb[d], fb[d], ub[d], m0, forms[1], True)
    return ratios


# ---------------------------------------------------------------------------------------------------------------------
# fronts
# ---------------------------------------------------------------------------------------------------------------------
FRONT_PARAMS = ('w_ih', 'w_hh', 'b_ih', 'b_hh', 'proj.w', 'proj.b', 'stop.w', 'stop.b')


def _rel_l2(got, ref):
    n = float(ref.norm())
    e = float((got.double() - ref).norm())
    if e != e:
        return float('inf')
    return e / n if n > 0 else (0.0 if e == 0 else float('inf'))


def front_errors(inp, ref, got):
    e = dict(x=err_of(got['x'], ref['x']), s=err_of(got['s'], ref['s']), dzc=err_of(got['dzc'], ref['dzc']))
    for i, name in enumerate(FRONT_PARAMS):
        for j, vg in enumerate('vg'):
            a, b = got['grads'][2 * i + j], ref['grads'][2 * i + j]
            if vg == 'v' and b.dim() == 1:
                # a bias is a weight-normed tensor whose rows hold ONE element: w = g * sign(v), so dL/dv is identically 0
                # and what any arithmetic leaves there is the difference of two equal terms of size |g / v| |dL/dw|
                # (|dL/dw| = |dL/dg|).  That size is the scale its error is a fraction of; the reference's own 1e-17 is not.
                v, g = [t.double().view(-1) for t in inp['vg'][i]]
                scale = float((g / v * ref['grads'][2 * i + 1].view(-1)).abs().max())
                d = float((a.double() - b).abs().max())
                e['d%s_v.elem' % name] = d / scale if d == d else float('inf')
                continue
            e['d%s_%s.l2' % (name, vg)], e['d%s_%s.elem' % (name, vg)] = _rel_l2(a, b), err_of(a, b)
    return e


def front_floor(cell, inp, ref):
    """the fp32 run of ref_front against its float64 run"""
    return front_errors(inp, ref, ref_front(cell, inp['zc'], inp['vg'], inp['gx'], inp['gs'], dtype=torch.float32))


def check_front(case, inp, ref, floor, got, form='model', again=None):
    """got: dict(x, s, dzc, grads, frames_ok[, slab_rest_ok]).  Returns {output: error / floor}"""
    tag = (case, form)
    assert got['frames_ok'], ('guard frame: a store landed outside the frames', tag)
    errs = front_errors(inp, ref, got)
    ratios = {}
    for name, e in errs.items():
        ceil = CEIL_GRAD_L2 if name.endswith('.l2') else CEIL_GRAD_ELEM if name.endswith('.elem') else CEIL
        b = bound(margin_of(form, name), floor[name], ceil)
        assert 0 < b <= ceil, ('bound of ' + name, tag, b)
        assert e <= b, ('out of bound: ' + name, tag, e, floor[name])
        ratios[name] = e / max(floor[name], FLOOR_MIN)
    if again is not None:
        for k in ('x', 's', 'dzc', 'grads'):
            assert same_bits(got[k], again[k]), ('not reproducible: ' + k, tag)
    return ratios


_PREPARED = {}


def prepared_layer(case):
    """(inputs, float64 reference, floor) of a layer case, computed once per process and shared"""
    key = ('layer', case['id'])
    if key not in _PREPARED:
        inp = make_layer_inputs(case)
        ref = ref_lstm_layer(inp['pre'], inp['whh'], inp['valid'], inp['static'], inp['dy'])
        _PREPARED[key] = (inp, ref, layer_floor(case, inp, ref))
    return _PREPARED[key]


def prepared_front(case, cell):
    key = ('front', cell, case['id'])
    if key not in _PREPARED:
        inp = make_front_inputs(case, cell)
        ref = ref_front(cell, inp['zc'], inp['vg'], inp['gx'], inp['gs'])
        _PREPARED[key] = (inp, ref, front_floor(cell, inp, ref))
    return _PREPARED[key]


def merge_worst(table, form, ratios):
    row = table.setdefault(form, {})
    for k, v in ratios.items():
        row[k] = max(row.get(k, 0.0), v)
