"""The autograd block fuzz  --  TEST INFRASTRUCTURE (no test functions).

The layer between the kernels and the networks: the ``torch.autograd.Function``s of audiogan_amd/ops.py, recurrent.py,
convnets.py, extras.py and losses.py, and the gradient bookkeeping of common.py (WNGroup, grad_target, frozen,
network_backward, finish_pending).  Each Function is called DIRECTLY with a hand-built GTrunk / DConvStack / DHead, at
the smallest shapes that select a branch, under every gradient route, and held to a float64 reference written in plain
torch double with torch's own autograd.

  case tables        FAMILIES[name].cases()            the structural classes of DESIGN.md section 2
  float64 reference  Family.ref(case, params, inputs)  w = g v / ||v|| per row, conv1d / conv_transpose1d, LeakyReLU at
                                                       K.LEAKY_SLOPE, length masks, the dense residual concatenation,
                                                       nn.LSTM semantics with zeroed padded steps, masked BCE
  runner / checker   run_block / ref_block / check_block / check_routes / sweep / check_cache
  branch predicates  conv_o1_ok / rowdot_ok_sizes / lstm_step_ok / lstm_bwd_seq, restated from sizes alone (Family.classes)
  coverage           assert_coverage(name, cases)      one assertion per family

tests/test_block_fuzz.py runs ``sweep`` on the HIP kernels, tests/test_block_fuzz_host.py on the CPU model of the kernels
(tests/kernel_model.py through ``install_model``) and on mutants of the Functions, each of which the sweep must reject.

The bound rule is DESIGN.md section 2's, unchanged: per case, route and tensor the FLOOR is the error of the same block
run on the CPU kernel model in fp32 against the float64 reference, as a fraction of the reference tensor's largest
magnitude and not below 2^-24; the bound is MARGIN x floor, never above CEIL of the scale.  Cases in bf16 precision or on
bf16 storage (GPU only: the model has neither) are held to the float64 block with contractions and stored tensors rounded
as oracle.bf16_mode(store=...) states (``Contract``), at the tolerances tests/test_bf16.py declares.
"""
import collections
import contextlib
import types
import warnings

import torch
import torch.nn.functional as F

SLOPE = 0.01                 # K.LEAKY_SLOPE (asserted equal in install_model / the GPU test)
MARGIN = 16.0
MARGIN_MAX = 64.0
# family -> a margin above 16, at most MARGIN_MAX, with its reason (none needed so far: see profiles/block_fuzz.txt)
MARGINS = {}
CEIL = 1e-4
FLOOR_MIN = 2.0 ** -24

# route -> start: how .grad is preset (None / 'zero' / 'rand' / 'some': zeros on half the parameters / 'nc': non-contiguous
# zeros); scope: the backward runs inside common.network_backward(); twice: two applications, one backward; freeze: 'all'
# or 'part' of the parameters under common.frozen, `when` the FORWARD runs (the input-gradient passes) or when the BACKWARD
# runs, with the forward unfrozen (the stopper-only order of train.g_step_full: backward, then a second backward of the
# same graph under losses.only_stopper_trains); nox: no input takes a gradient
def _route(start=None, scope=False, twice=False, freeze=None, when='fwd', nox=False):
    return dict(start=start, scope=scope, twice=twice, freeze=freeze, when=when, nox=nox)


ROUTE = collections.OrderedDict([
    ('fresh', _route()), ('direct0', _route('zero')), ('direct_rand', _route('rand')), ('direct_some', _route('some')),
    ('scope', _route('zero', scope=True)), ('scope_rand', _route('rand', scope=True)),
    ('twice', _route('rand', scope=True, twice=True)), ('frozen', _route('rand', freeze='all')),
    ('part', _route(freeze='part')), ('part_fwd0', _route('zero', freeze='part')), ('part_fwd_rand', _route('rand', freeze='part')),
    ('part_bwd0', _route('zero', freeze='part', when='bwd')), ('part_bwd_rand', _route('rand', freeze='part', when='bwd')),
    ('part_bwd_scope', _route('rand', scope=True, freeze='part', when='bwd')),
    ('nograd_x', _route(nox=True)), ('noncontig', _route('nc'))])
ROUTES = tuple(ROUTE)
PART_ROUTES = tuple(r for r in ROUTES if ROUTE[r]['freeze'] == 'part')
# routes whose parameter gradients, from a zero start, must have the bits of 'fresh'
RUN_TWICE = ('fresh', 'direct_rand', 'twice', 'part_bwd_rand')
SAME_AS_FRESH = ('direct0', 'direct_some', 'scope', 'nograd_x', 'noncontig')


def margin_of(fam):
    m = MARGINS.get(fam, MARGIN)
    assert MARGIN <= m <= MARGIN_MAX
    return m


def bound(margin, floor, ceil=CEIL):
    return min(margin * max(floor, FLOOR_MIN), ceil)


def same_bits(a, b):
    if a is None or b is None:
        return a is None and b is None
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(same_bits(x, y) for x, y in zip(a, b))
    if a.dtype not in (torch.float32, torch.bfloat16):
        return a.shape == b.shape and torch.equal(a, b)
    bits = torch.int32 if a.dtype == torch.float32 else torch.int16
    return a.shape == b.shape and torch.equal(a.contiguous().view(bits), b.contiguous().view(bits))


def same_value_bits(a, b):
    """bit equality up to the sign of zero (0 + (-0) = +0: an accumulation into a zero start may flip it)"""
    if a is None or b is None:
        return a is None and b is None
    return a.shape == b.shape and torch.equal(a, b) and not bool(torch.isnan(a).any())


def merge_worst(table, form, ratios):
    row = table.setdefault(form, {})
    for k, v in ratios.items():
        row[k] = max(row.get(k, 0.0), v)


# ---------------------------------------------------------------------------------------------------------------------
# the CPU model of the kernels, with the deferral scopes kernels.py keeps on the host
# ---------------------------------------------------------------------------------------------------------------------
def install_model(monkeypatch):
    """tests/kernel_model.py in place of audiogan_amd.kernels, plus a host model of the deferral scopes
    (kernels.deferred_reduces / reduces_outer / flush_reduces): the model's sums are final at once, but WHETHER a
    network-level scope is open decides how common.WNGroup.backward routes its weight-norm backward (joined to the
    scope's one launch, or on the spot), and that routing is what the 'scope' and 'twice' routes are about."""
    import audiogan_amd.kernels as K
    from tests import kernel_model as KM
    assert KM.LEAKY_SLOPE == SLOPE == K.LEAKY_SLOPE
    KM.install(monkeypatch)
    st = dict(keep=None, outer=False, depth=0)

    class deferred_reduces(object):
        def __init__(self, outer=False):
            self.outer, self.role = bool(outer), None

        def __enter__(self):
            if st['keep'] is None:
                st['keep'], st['outer'], st['depth'] = [], self.outer, 0
                self.role = 'owner'
            elif self.outer:
                self.role = 'nested'
            else:
                st['depth'] += 1
                self.role = 'inner'
            return self

        def __exit__(self, *exc):
            if self.role == 'inner':
                st['depth'] -= 1
            elif self.role == 'owner':
                st['keep'], st['outer'], st['depth'] = None, False, 0
            return False

    monkeypatch.setattr(K, 'deferred_reduces', deferred_reduces)
    monkeypatch.setattr(K, 'reduces_outer', lambda: st['keep'] is not None and st['outer'])
    monkeypatch.setattr(K, 'reduces_recording', lambda: st['keep'] is not None and (st['depth'] > 0 or not st['outer']))
    monkeypatch.setattr(K, 'flush_reduces', lambda: None)
    return K


class counting(object):
    """``with counting(K, names) as n``: n[name] = calls of K.<name> inside the block (which branch a Function took);
    n[(name, act)]: those with the keyword ``act`` = act"""

    def __init__(self, K, names):
        self.K, self.names, self.n = K, names, collections.Counter()

    def __enter__(self):
        self.old = {k: getattr(self.K, k) for k in self.names}
        for k, f in self.old.items():
            setattr(self.K, k, lambda *a, _f=f, _k=k, **kw: (self.n.update([_k, (_k, kw.get('act'))]), _f(*a, **kw))[1])
        return self.n

    def __exit__(self, *exc):
        for k, f in self.old.items():
            setattr(self.K, k, f)


# ---------------------------------------------------------------------------------------------------------------------
# pieces of the float64 references
# ---------------------------------------------------------------------------------------------------------------------
def wn(v, g):
    """weight norm over dim 0: w = g v / ||v|| per row (a bias is a column of one-element rows: w = g sign(v))"""
    rows = v.size(0)
    n = v.reshape(rows, -1).norm(dim=1).view(rows, *([1] * (v.dim() - 1)))
    return v * (g.reshape(n.shape) / n)


def leaky(t):
    return torch.where(t > 0, t, t * SLOPE)


def len_mask(lens, L, dtype):
    return (torch.arange(L).view(1, L) < lens.view(-1, 1)).to(dtype)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ---- AG_PREC_BF16 and bf16 storage, as oracle.bf16_mode(store=...) states them ---------------------------------------------
#   a contraction   y = op(rnd(x), rnd(w)) (+ bias, exact); backward: the gradient entering it is rounded, so
#                   dx = op_bwd_data(rnd(dy), rnd(w)), dw = op_bwd_weight(rnd(dy), rnd(x)), dbias = sum(dy)
#   a stored tensor (bf16 storage) is rounded where it is written, value and gradient; a stored activation act(pre): the
#                   value after the activation, the gradient after the activation's derivative
def rnd(t):
    return t.float().bfloat16().to(t.dtype)


class _RoundFwd(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return rnd(x)

    @staticmethod
    def backward(ctx, g):
        return g


class _RoundBwd(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return rnd(g)


class Contract(object):
    """how a reference contracts and stores: mode 'f32' (exact), 'bf16' (rounded contractions), 'store' (and bf16 storage)"""

    def __init__(self, mode):
        assert mode in ('f32', 'bf16', 'store')
        self.mode = mode

    def lin(self, x, w):
        """x @ w^T"""
        if self.mode == 'f32':
            return x @ w.t()
        return _RoundBwd.apply(_RoundFwd.apply(x) @ _RoundFwd.apply(w).t())

    def st(self, x):
        return _RoundBwd.apply(_RoundFwd.apply(x)) if self.mode == 'store' else x

    def st_act(self, pre, act):
        return _RoundFwd.apply(act(_RoundBwd.apply(pre))) if self.mode == 'store' else act(pre)


def contract_of(case):
    return Contract(dict(f32='f32', add='bf16', gate='store', widen='store', x16='store')[case.get('mode', 'f32')])


def is_f32(case):
    return case.get('mode', 'f32') == 'f32'


# the tolerances tests/test_bf16.py holds the corresponding module comparisons to: activations, logits
# and input gradients 1e-2 of the largest magnitude elementwise and 3e-3 in relative L2 (5e-3 on bf16 storage); parameter
# gradients 5e-2 elementwise (8e-2 on bf16 storage) and 2e-2 in relative L2, the weight-norm gains 5e-2 in L2; the
# v-gradient of a bias (identically 0) is not compared
BF16_ACT = dict(elem=1e-2, l2=3e-3, l2_store=5e-3)
BF16_PAR = dict(elem=5e-2, elem_store=8e-2, l2=2e-2, l2_gain=5e-2)


def _wn_pair(gen, shape):
    """(v, g) of one weight-normed tensor, in the shapes modules._register_wn gives them"""
    rows = shape[0]
    if len(shape) == 1:
        v = torch.randn(rows, generator=gen)
        v = torch.where(v.abs() < 0.2, v.sign() * 0.2 + (v == 0).float() * 0.2, v)     # (g / v stays moderate)
        return v, torch.rand(rows, generator=gen) * 0.3 + 0.05
    v = torch.randn(*shape, generator=gen)
    return v, torch.rand(rows, *([1] * (len(shape) - 1)), generator=gen) + 0.5       # (row norms of w in [0.5, 1.5])


def _nc_copy(t):
    """a non-contiguous view holding t's values (every other element of a buffer twice as wide)"""
    wide = torch.zeros(*t.shape[:-1], 2 * t.shape[-1], dtype=t.dtype, device=t.device)
    wide[..., ::2] = t
    return wide[..., ::2]


def _nc_like(t):
    """a zero tensor of t's shape that is not contiguous (when it has more than one element)"""
    return torch.zeros(2 * t.numel(), dtype=t.dtype, device=t.device)[::2].view(t.shape)


# ---------------------------------------------------------------------------------------------------------------------
# families
# ---------------------------------------------------------------------------------------------------------------------
class Family(object):
    """one Function (with what stands in front of it) and its table.

    values(case) -> dict(params=[fp32 CPU tensors in Function order], names=[...], bias_v={index of a bias's v: index
                    of its g}, xs=[differentiable inputs], xs2=[a second set, for 'twice'], req=[which inputs take a
                    gradient], cots=[one per output, None: no gradient arrives], cots2=[...], starts=[random .grad
                    starts])
    build(case, params, dev, vals) -> (apply(*xs) -> tuple of outputs, group or None)
    place(case, i, value, dev) -> input i on the device in the layout the case asks for
    ref(case, p64, xs64, vals) -> tuple of float64 outputs
    part(case, vals) -> indices of the parameters frozen under the 'part' route"""
    name = None
    routes = ROUTES
    out_names = None

    def place(self, case, i, value, dev):
        return value.to(dev).clone()

    def part(self, case, vals):
        n = len(vals['params'])
        return list(range(0, n - 2))            # all but the last weight-normed tensor (the stopper-only pattern)

    def cot(self, case, j, c, dev):
        return c.to(dev)

    def starts(self, vals, seed):
        gen = _gen(seed)
        return [torch.randn(p.shape, generator=gen) * 0.5 for p in vals['params']]

    def after_run(self, case, route):
        pass

    def some(self, case, vals):
        return len(vals['params']) // 4 * 2


def _finish_vals(fam, case, vals, seed):
    vals.setdefault('xs2', vals['xs'])
    vals.setdefault('cots2', vals['cots'])
    vals.setdefault('req', [True] * len(vals['xs']))
    vals.setdefault('bias_v', {})
    vals['starts'] = fam.starts(vals, seed + 7)
    return vals


_VALS = {}


def values(fam, case):
    key = (fam.name, case['id'])
    if key not in _VALS:
        seed = 1000 + 7919 * sorted(FAMILIES).index(fam.name) + 31 * case['n']
        _VALS[key] = _finish_vals(fam, case, fam.values(case, seed), seed)
    return _VALS[key]


# ---- 1. GTrunkFn -----------------------------------------------------------------------------------------------------
def conv_o1_ok(kind, cout, K_, stride, pad):
    return kind == 'conv' and cout == 1 and stride == 1 and K_ <= 9 and 2 * pad == K_ - 1


class GTrunkFam(Family):
    name = 'gtrunk'

    def cases(self):
        t = [dict(B=1, L=64, bn=[(17, 8, 6, 4)], fk=9, place='contig'),
             dict(B=3, L=96, bn=[(17, 8, 5, 3), (9, 4, 6, 4), (5, 2, 4, 2)], fk=11, place='inplace'),
             dict(B=3, L=64, bn=[(9, 4, 4, 3), (5, 2, 5, 3), (17, 8, 3, 2)], fk=7, place='view_big'),
             dict(B=1, L=96, bn=[(5, 2, 4, 2)], fk=11, place='view_off'),
             dict(B=3, L=64, bn=[(5, 2, 3, 2), (17, 8, 4, 3), (9, 4, 5, 2)], fk=9, place='inplace'),
             dict(B=1, L=96, bn=[(9, 4, 5, 3)], fk=5, place='inplace')]
        for n, c in enumerate(t):
            c['n'], c['id'] = n, 'gtrunk%d' % n
            c['ctot'] = 1 + sum(o for _, _, _, o in c['bn'])
        return t

    def classes(self, c):
        s = {('place', c['place']), ('nbn', len(c['bn'])), ('B', c['B']), ('L', c['L']),
             ('final', 'o1' if conv_o1_ok('conv', 1, c['fk'], 1, (c['fk'] - 1) // 2) else 'engine')}
        cin = 1
        for i, (k, st, hid, out) in enumerate(c['bn']):
            s.add(('ks', k, st))
            s.add(('res', cin >= out))
            assert (cin >= out) == (i > 0), 'the first bottleneck has cin < cout, the later ones cin >= cout'
            cin += out
        return s

    REQUIRED = ({('place', p) for p in ('inplace', 'contig', 'view_big', 'view_off')} | {('nbn', 1), ('nbn', 3)}
                | {('ks', 17, 8), ('ks', 9, 4), ('ks', 5, 2)} | {('res', True), ('res', False)}
                | {('final', 'o1'), ('final', 'engine')} | {('B', 1), ('B', 3), ('L', 64), ('L', 96)})

    def _shapes(self, c):
        out, cin = [], 1
        for i, (k, st, hid, o) in enumerate(c['bn']):
            out += [('bn%d.conv.w' % i, (hid, cin, k)), ('bn%d.conv.b' % i, (hid,)),
                    ('bn%d.deconv.w' % i, (hid, o, k - 1)), ('bn%d.deconv.b' % i, (o,))]
            cin += o
        return out + [('final.w', (1, cin, c['fk'])), ('final.b', (1,))]

    def values(self, c, seed):
        gen = _gen(seed)
        params, names, bias_v = [], [], {}
        for nm, sh in self._shapes(c):
            v, g = _wn_pair(gen, sh)
            if len(sh) == 1:
                bias_v[len(params)] = len(params) + 1
            params += [v, g]
            names += [nm + '_v', nm + '_g']
        B, L = c['B'], c['L']
        rn = lambda *s: torch.randn(*s, generator=gen)        # noqa: E731
        return dict(params=params, names=names, bias_v=bias_v, xs=[rn(B, L)], xs2=[rn(B, L)], cots=[rn(B, L)],
                    cots2=[rn(B, L)])

    def specs(self, c):
        from audiogan_amd.ops import ConvSpec
        bn, cin = [], 1
        for k, st, hid, o in c['bn']:
            bn.append((ConvSpec('conv', cin, hid, k, st, (k - 1) // 2), ConvSpec('convT', hid, o, k - 1, st, st // 2)))
            cin += o
        return bn, ConvSpec('conv', cin, 1, c['fk'], 1, (c['fk'] - 1) // 2)

    def build(self, c, params, dev, vals):
        from audiogan_amd import ops
        bn, fin = self.specs(c)
        trunk = ops.GTrunk(bn, fin)
        it = iter(params)
        for cs, ds in bn:
            for sp in (cs, ds):
                trunk.group.add(next(it), next(it), stride=sp.stride, engine=True, pad=sp.pad)
                trunk.group.add(next(it), next(it))
        trunk.group.add(next(it), next(it), stride=1, engine=True)
        trunk.group.add(next(it), next(it))
        assert trunk.ctot == c['ctot'] and trunk.group.params() == list(params)
        return (lambda x: (ops.GTrunkFn.apply(x, trunk, *trunk.group.params()),)), trunk.group

    def place(self, c, i, value, dev):
        B, L, ctot = c['B'], c['L'], c['ctot']
        if c['place'] == 'contig':
            return value.to(dev).clone()
        if c['place'] == 'inplace':           # channel 0 of a fresh [B, ctot, L] slab
            x = torch.full((B, ctot, L), float('nan'), device=dev)[:, 0, :]
        elif c['place'] == 'view_big':        # the right strides, offset 0, in a LARGER storage: must be copied
            x = torch.full((B * ctot * L + 16,), float('nan'), device=dev).as_strided((B, L), (ctot * L, 1), 0)
        else:                                 # the right strides at a non-zero offset: must be copied
            x = torch.full((B * ctot * L + 4,), float('nan'), device=dev).as_strided((B, L), (ctot * L, 1), 4)
        x.copy_(value)
        LAST['bases'].append((x, x.as_strided((x.untyped_storage().nbytes() // 4,), (1,), 0)))
        return x

    def after_run(self, c, route):
        """'inplace': the Function worked in the storage it was handed (channels 1.. of the slab are written); the two
        views: it copied (everything around the input is still NaN)"""
        B, L, ctot = c['B'], c['L'], c['ctot']
        for x, flat in LAST['bases']:
            if c['place'] == 'inplace':
                assert not bool(torch.isnan(flat).any()), ('the trunk did not take its input in place', c['id'], route)
            else:
                off = x.storage_offset()
                own = torch.zeros(flat.numel(), dtype=torch.bool, device=flat.device)
                own.as_strided((B, L), (ctot * L, 1), off).fill_(True)
                assert bool(torch.isnan(flat[~own]).all()) and not bool(torch.isnan(flat[own]).any()), \
                    ('the trunk wrote into a storage that is not a fresh slab', c['id'], route)

    def ref(self, c, p, xs, vals):
        feat = xs[0].unsqueeze(1)
        cin, q = 1, 0
        for k, st, hid, o in c['bn']:
            wc, bc, wd, bd = (wn(p[q + 2 * j], p[q + 2 * j + 1]) for j in range(4))
            q += 8
            h = leaky(F.conv1d(feat, wc, bc, st, (k - 1) // 2))
            y = F.conv_transpose1d(h, wd, bd, st, st // 2)
            if cin >= o:
                y = y + feat[:, cin - o:cin]            # the dense residual: the newest `o` channels
            feat = torch.cat([feat, leaky(y)], 1)
            cin += o
        wf, bf = wn(p[q], p[q + 1]), wn(p[q + 2], p[q + 3])
        return (F.conv1d(feat, wf, bf, 1, (c['fk'] - 1) // 2).squeeze(1),)


# ---- 2. DConvStackFn -------------------------------------------------------------------------------------------------
class DConvStackFam(Family):
    name = 'dconv'

    def cases(self):
        L4 = [(4, 7, 2, 3), (6, 7, 2, 3), (5, 7, 2, 3), (8, 7, 2, 3)]
        lens = [32, 9, 20]                  # a full clip, one whose length after four layers is 1, one between
        t = [dict(layers=L4[:1], pat=(1,), ncg=False),
             dict(layers=L4[:2], pat=(0, 1), ncg=False),
             dict(layers=L4[:2], pat=(1, 1), ncg=True),
             dict(layers=L4, pat=(0, 0, 0, 1), ncg=False),            # train.d_backward_late: the last output only
             dict(layers=L4, pat=(1, 1, 1, 1), ncg=False),            # feature matching (d_step_full / g_step_full)
             dict(layers=L4, pat=(0, 1, 0, 0), ncg=False),            # one middle layer: the top layers `continue`
             dict(layers=L4, pat=(0, 0, 1, 0), ncg=True),
             dict(layers=L4, pat=(1, 0, 0, 1), ncg=True)]             # gated epilogues, then an ungated layer
        for n, c in enumerate(t):
            c.update(n=n, id='dconv%d' % n, B=3, L=32, lens=lens)
        return t

    def lens_list(self, c):
        out, prod = [], 1
        for _, _, st, _ in c['layers']:
            prod *= st
            out.append(torch.tensor([(l + prod - 1) // prod for l in c['lens']], dtype=torch.long))
        return out

    def classes(self, c):
        pat, n = c['pat'], len(c['layers'])
        s = {('depth', n), ('ncg', c['ncg'])}
        if pat == (0,) * (n - 1) + (1,):
            s.add('last_only')
        if all(pat) and n > 1:
            s.add('all')
        if n > 2 and sum(pat) == 1 and not pat[-1] and not pat[0]:
            s.add('middle_only')
        if n > 2 and pat[0] and pat[-1] and not any(pat[1:-1]):
            s.add('first_plus_last')
        ll = self.lens_list(c)[-1].tolist()
        if n == 4 and 1 in ll and c['L'] // 16 in ll:
            s.add('last_len_1_and_full')
        return s

    REQUIRED = {('depth', 1), ('depth', 2), ('depth', 4), ('ncg', True), ('ncg', False), 'last_only', 'all', 'middle_only',
                'first_plus_last', 'last_len_1_and_full'}

    def values(self, c, seed):
        gen = _gen(seed)
        params, names, bias_v, cin = [], [], {}, 1
        for i, (co, k, st, pd) in enumerate(c['layers']):
            for nm, sh in (('l%d.w' % i, (co, cin, k)), ('l%d.b' % i, (co,))):
                v, g = _wn_pair(gen, sh)
                if len(sh) == 1:
                    bias_v[len(params)] = len(params) + 1
                params += [v, g]
                names += [nm + '_v', nm + '_g']
            cin = co
        B, L = c['B'], c['L']
        rn = lambda *s: torch.randn(*s, generator=gen)        # noqa: E731
        shapes, l = [], L
        for co, k, st, pd in c['layers']:
            l = (l + 2 * pd - k) // st + 1
            shapes.append((B, co, l))
        cots = [rn(*s) if on else None for s, on in zip(shapes, c['pat'])]
        cots2 = [rn(*s) if on else None for s, on in zip(shapes, c['pat'])]
        return dict(params=params, names=names, bias_v=bias_v, xs=[rn(B, L)], xs2=[rn(B, L)], cots=cots, cots2=cots2)

    def cot(self, c, j, t, dev):
        return _nc_copy(t.to(dev)) if c['ncg'] else t.to(dev)

    def build(self, c, params, dev, vals):
        from audiogan_amd import ops
        specs = [ops.ConvSpec('conv', ci, co, k, st, pd)
                 for ci, (co, k, st, pd) in zip([1] + [l[0] for l in c['layers'][:-1]], c['layers'])]
        stack = ops.DConvStack(specs)
        it = iter(params)
        for sp in specs:
            stack.group.add(next(it), next(it), stride=sp.stride, engine=True, pad=sp.pad)
            stack.group.add(next(it), next(it))
        ll = [l.to(dev) for l in self.lens_list(c)]
        LAST['lens_list'] = ll
        return (lambda x: tuple(ops.DConvStackFn.apply(x, stack, ll, *stack.group.params()))), stack.group

    def ref(self, c, p, xs, vals):
        a, outs = xs[0].unsqueeze(1), []
        for i, ((co, k, st, pd), ln) in enumerate(zip(c['layers'], self.lens_list(c))):
            w, b = wn(p[4 * i], p[4 * i + 1]), wn(p[4 * i + 2], p[4 * i + 3])
            a = leaky(F.conv1d(a, w, b, st, pd))
            a = a * len_mask(ln, a.size(2), a.dtype).unsqueeze(1)
            outs.append(a)
        return tuple(outs)


LAST = {'bases': []}       # what the latest build() handed its Function besides tensors (the host mutants look things up here)


# ---- 3. TimeMajorFn + DHeadFn ----------------------------------------------------------------------------------------
def rowdot_ok_sizes(n_out):
    """ops.DHeadFn takes the one-wave-per-row kernels iff the classifier has ONE output (hmid is contiguous and w1 has as
    many elements as hmid has columns exactly then)"""
    return n_out == 1


class DHeadFam(Family):
    name = 'dhead'

    def cases(self):
        t = []
        for n_res, n_out, (T, B), S in [(0, 1, (1, 1), 16), (0, 3, (7, 1), 16), (1, 1, (1, 7), 16), (1, 3, (5, 13), 16),
                                        (2, 1, (5, 13), 16), (2, 3, (7, 1), 16), (2, 1, (1, 1), 64), (2, 3, (5, 13), 48)]:
            t.append(dict(n_res=n_res, n_out=n_out, T=T, B=B, S=S, mode='f32'))
        # bf16 precision: 'add' fp32 rows; bf16 rows: 'gate' at state 64 (gemm_h_ok holds), 'widen' at 48 (it refuses)
        for mode, n_res, n_out, (T, B), S in [('add', 2, 1, (5, 13), 16), ('add', 1, 3, (7, 1), 16),
                                              ('gate', 2, 1, (5, 13), 64), ('gate', 1, 3, (7, 1), 64), ('gate', 2, 3, (16, 8), 64),
                                              ('widen', 2, 1, (5, 13), 48), ('widen', 2, 3, (7, 1), 48)]:
            t.append(dict(n_res=n_res, n_out=n_out, T=T, B=B, S=S, mode=mode))
        for n, c in enumerate(t):
            c.update(n=n, id='dhead%d' % n, M=c['T'] * c['B'])
        return t

    def classes(self, c):
        return {('n_res', c['n_res']), ('cls', 'rowdot' if rowdot_ok_sizes(c['n_out']) else 'gemm'), ('M', c['M']),
                ('skip', dict(f32='fold', add='add', gate='gate', widen='gate')[c['mode']], c['n_res'] > 0),
                ('fold_identity', c['mode'] == 'f32' and c['n_res'] > 1), ('rows16', c['mode'] in ('gate', 'widen'), c['S'] % 64 == 0)}

    REQUIRED = {('n_res', 0), ('n_res', 1), ('n_res', 2), ('cls', 'rowdot'), ('cls', 'gemm'), ('M', 1), ('M', 7), ('M', 65),
                ('skip', 'fold', True), ('skip', 'add', True), ('skip', 'gate', True), ('fold_identity', True),
                ('rows16', True, True), ('rows16', True, False), ('rows16', False, False)}

    def values(self, c, seed):
        gen = _gen(seed)
        S, params, names, bias_v = c['S'], [], [], {}
        shapes = []
        for i in range(c['n_res']):
            shapes += [('res%d.w' % i, (S, S)), ('res%d.b' % i, (S,))]
        shapes += [('cls0.w', (S // 2, S)), ('cls0.b', (S // 2,)), ('cls1.w', (c['n_out'], S // 2)), ('cls1.b', (c['n_out'],))]
        for nm, sh in shapes:
            v, g = _wn_pair(gen, sh)
            if len(sh) == 1:
                bias_v[len(params)] = len(params) + 1
            params += [v, g]
            names += [nm + '_v', nm + '_g']
        rn = lambda *s: torch.randn(*s, generator=gen)        # noqa: E731
        B, T, M = c['B'], c['T'], c['M']
        return dict(params=params, names=names, bias_v=bias_v, xs=[rn(B, S, T)], xs2=[rn(B, S, T)],
                    cots=[rn(M, c['n_out'])], cots2=[rn(M, c['n_out'])])

    def build(self, c, params, dev, vals):
        from audiogan_amd import ops
        head = ops.DHead(c['n_res'])
        it = iter(params)
        for _ in range(len(params) // 2):
            head.group.add(next(it), next(it))

        def apply(a):
            seq = ops.TimeMajorFn.apply(a, c['mode'] in ('gate', 'widen'))
            return (ops.DHeadFn.apply(seq.reshape(c['M'], c['S']), head, *head.group.params()),)
        return apply, head.group

    def ref(self, c, p, xs, vals):
        ct = contract_of(c)
        a = ct.st(xs[0].permute(2, 0, 1).reshape(c['M'], c['S']))
        q = 0
        for _ in range(c['n_res']):
            a = ct.st_act(ct.lin(a, wn(p[q], p[q + 1])) + wn(p[q + 2], p[q + 3]) + a, leaky)
            q += 4
        h = ct.st_act(ct.lin(a, wn(p[q], p[q + 1])) + wn(p[q + 2], p[q + 3]), leaky)
        return (ct.lin(h, wn(p[q + 4], p[q + 5])) + wn(p[q + 6], p[q + 7]),)


# ---- 4. LSTMSeqFn ----------------------------------------------------------------------------------------------------
def lstm_step_ok(B, H):
    return B <= 256 and H % 8 == 0


def lstm_bwd_seq(B, H):
    """recurrent.LSTMSeqFn.backward hands the whole backward through time to K.lstm_seq_bwd (else: one cell launch and
    one product per step from Python)"""
    return B <= 256 and H % 2 == 0


class LSTMFam(Family):
    name = 'lstm'

    def cases(self):
        t = []
        # cls: 'persist' fused step kernels + the persistent launches (H = 64); 'fused' the step kernels without them;
        # 'loop' neither (odd H); 'loop_fwd' the Python forward loop with K.lstm_seq_bwd (H % 8 != 0, even); 'wide' B = 257
        for cls, B, H, T, ndir, st, need_ds, lens in [
                ('persist', 4, 64, 3, 2, True, True, 'ragged'), ('persist', 4, 64, 3, 1, False, False, None),
                ('persist', 3, 64, 1, 2, True, False, 'ragged'), ('persist', 4, 64, 3, 2, False, False, 'ragged'),
                ('fused', 4, 24, 3, 2, True, True, 'ragged'), ('fused', 3, 8, 1, 1, True, True, None),
                ('fused', 4, 24, 3, 2, False, False, None),
                ('loop', 4, 25, 3, 2, True, True, 'ragged'), ('loop', 3, 25, 1, 1, False, False, None),
                ('loop', 4, 25, 3, 2, True, False, None),
                ('loop_fwd', 4, 10, 3, 2, True, True, 'ragged'),
                ('wide', 257, 4, 2, 2, True, True, 'ragged'), ('wide', 257, 4, 2, 1, False, False, None)]:
            t.append(dict(cls=cls, B=B, H=H, T=T, ndir=ndir, static=st, need_ds=need_ds, lens=lens, Fx=8 if H % 8 == 0 else 5,
                          Fc=4, mode='f32'))
        # bf16-stored x at H = 64 (bf16 precision): y, dy and dx are bfloat16, the large products run on ag_gemm_h
        t.append(dict(cls='persist', B=4, H=64, T=3, ndir=2, static=True, need_ds=True, lens='ragged', Fx=64, Fc=4, mode='x16'))
        t.append(dict(cls='persist', B=4, H=64, T=3, ndir=1, static=False, need_ds=False, lens=None, Fx=8, Fc=4, mode='x16'))
        for n, c in enumerate(t):
            c.update(n=n, id='lstm%d' % n)
        return t

    def lengths(self, c):
        if c['lens'] is None:
            return None
        T, B = c['T'], c['B']
        v = torch.tensor(([T, 0, 1] + [max(1, T - 1), T] * B)[:B], dtype=torch.long)
        return v

    def classes(self, c):
        B, H = c['B'], c['H']
        s = {('cls', c['cls']), ('ndir', c['ndir']), ('T', c['T']), ('static', c['static'], c['need_ds']),
             ('lens', c['lens']), ('fwd_fused', lstm_step_ok(B, H)), ('bwd_seq', lstm_bwd_seq(B, H)), ('x16', c['mode'] == 'x16')}
        want = dict(persist=(True, True), fused=(True, True), loop=(False, False), loop_fwd=(False, True), wide=(False, False))
        assert (lstm_step_ok(B, H), lstm_bwd_seq(B, H)) == want[c['cls']], c
        if c['lens'] is not None:
            v = self.lengths(c).tolist()
            if 0 in v and 1 in v and c['T'] in v:
                s.add('lens_0_1_T')
        return s

    REQUIRED = ({('cls', k) for k in ('persist', 'fused', 'loop', 'loop_fwd', 'wide')} | {('ndir', 1), ('ndir', 2), ('T', 1), ('T', 3)}
                | {('static', False, False), ('static', True, True), ('static', True, False)} | {('lens', None), ('lens', 'ragged')}
                | {'lens_0_1_T', ('x16', True), ('x16', False)})

    def values(self, c, seed):
        gen = _gen(seed)
        rn = lambda *s: torch.randn(*s, generator=gen)        # noqa: E731
        B, H, T, Fx = c['B'], c['H'], c['T'], c['Fx']
        Fc = c['Fc'] if c['static'] else 0
        params, names = [], []
        for d in range(c['ndir']):
            params += [rn(4 * H, Fx + Fc) / (Fx + Fc) ** 0.5, rn(4 * H, H) / H ** 0.5, rn(4 * H) * 0.2, rn(4 * H) * 0.2]
            names += ['d%d.%s' % (d, k) for k in ('w_ih', 'w_hh', 'b_ih', 'b_hh')]
        xs, xs2, req = [rn(T, B, Fx)], [rn(T, B, Fx)], [True]
        if c['static']:
            xs.append(rn(B, Fc)); xs2.append(rn(B, Fc)); req.append(c['need_ds'])
        D = c['ndir'] * H
        return dict(params=params, names=names, xs=xs, xs2=xs2, req=req, cots=[rn(T, B, D)], cots2=[rn(T, B, D)])

    def part(self, c, vals):
        return list(range(4, len(vals['params'])))          # direction 1 frozen ...

    def some(self, c, vals):
        return 4 if c['ndir'] == 2 else 2           # direction 0 / half a direction (which cannot go direct alone)

    def place(self, c, i, value, dev):
        x = value.to(dev).clone()
        return x.to(torch.bfloat16) if (c['mode'] == 'x16' and i == 0) else x

    def cot(self, c, j, t, dev):
        return t.to(dev).to(torch.bfloat16) if c['mode'] == 'x16' else t.to(dev)

    def build(self, c, params, dev, vals):
        from audiogan_amd import ops
        ln = self.lengths(c)
        ln = ln.to(dev) if ln is not None else None

        def apply(x, static=None):
            return (ops.LSTMSeqFn.apply(x, ln, c['ndir'], static, *params),)
        return apply, None

    def ref(self, c, p, xs, vals):
        x = xs[0]
        T, B, _ = x.shape
        H, ln = c['H'], self.lengths(c)
        ct = contract_of(c)
        x = ct.st(x)
        inp = torch.cat([x, xs[1].unsqueeze(0).expand(T, B, xs[1].size(1))], 2) if c['static'] else x
        ys = []
        for d in range(c['ndir']):
            w_ih, w_hh, b_ih, b_hh = p[4 * d:4 * d + 4]
            h = c_ = torch.zeros(B, H, dtype=x.dtype)
            out = [None] * T
            for k in range(T):
                t = k if d == 0 else T - 1 - k
                g = ct.lin(inp[t], w_ih) + ct.lin(h, w_hh) + b_ih + b_hh
                i, f, gg, o = torch.sigmoid(g[:, :H]), torch.sigmoid(g[:, H:2 * H]), torch.tanh(g[:, 2 * H:3 * H]), \
                    torch.sigmoid(g[:, 3 * H:])
                c2 = f * c_ + i * gg
                h2 = o * torch.tanh(c2)
                live = (t < ln).view(B, 1) if ln is not None else torch.ones(B, 1, dtype=torch.bool)
                c_, h, out[t] = torch.where(live, c2, c_), torch.where(live, h2, h), torch.where(live, h2, torch.zeros_like(h2))
            ys.append(torch.stack(out))
        return (ct.st(torch.cat(ys, 2)),)


# ---- 5. the small Functions -------------------------------------------------------------------------------------------
class SmallFam(Family):
    """Functions without parameters: one route, the subsets of ``needs_input_grad`` are cases"""
    name = 'small'
    routes = ('fresh',)

    def cases(self):
        t = [dict(op='buildzc', req=(True, True)), dict(op='buildzc', req=(True, False)), dict(op='buildzc', req=(False, True)),
             dict(op='critic_input'),
             dict(op='bce', view='t', target='scalar', nframes=True), dict(op='bce', view='t', target='rows', nframes=True),
             dict(op='bce', view='plain', target='scalar', nframes=False), dict(op='bce', view='t', target='rows', nframes=False),
             dict(op='moments', cots=(1, 1, 1)), dict(op='moments', cots=(0, 1, 0)), dict(op='moments', cots=(1, 0, 1)),
             dict(op='per_sample', nframes=True), dict(op='per_sample', nframes=False)]
        for n, c in enumerate(t):
            c.update(n=n, id='small%d_%s' % (n, c['op']))
        return t

    def classes(self, c):
        s = {('op', c['op'])}
        if c['op'] == 'buildzc':
            s.add(('zc_req', c['req']))
        if c['op'] == 'bce':
            s |= {('bce_view', c['view']), ('bce_target', c['target']), ('bce_nframes', c['nframes'])}
        return s

    REQUIRED = ({('op', o) for o in ('buildzc', 'critic_input', 'bce', 'moments', 'per_sample')}
                | {('zc_req', r) for r in ((True, True), (True, False), (False, True))}
                | {('bce_view', 't'), ('bce_target', 'scalar'), ('bce_target', 'rows'), ('bce_nframes', False)})

    def values(self, c, seed):
        gen = _gen(seed)
        rn = lambda *s: torch.randn(*s, generator=gen)        # noqa: E731
        op = c['op']
        if op == 'buildzc':
            B, T, ns, es = 3, 5, 6, 4
            return dict(params=[], names=[], xs=[rn(B, T, ns), rn(B, es)], req=list(c['req']), cots=[rn(T, B, ns + es)])
        if op == 'critic_input':
            B, L = 3, 40
            return dict(params=[], names=[], xs=[rn(B, L)], cots=[rn(B, L), None], noise=rn(B, L) * 0.1,
                        length=torch.tensor([40, 9, 23]), prods=(2, 4, 8))
        if op == 'bce':
            B, T = 5, 7
            return dict(params=[], names=[], xs=[rn(T, B) if c['view'] == 't' else rn(B, T)], cots=[rn(()), None],
                        target=torch.rand(B, generator=gen) if c['target'] == 'rows' else 0.9,
                        nframes=torch.tensor([7, 1, 3, 6, 2]) if c['nframes'] else None)
        if op == 'moments':
            B, C, L = 3, 5, 12
            h = rn(B, C, L)
            lens = torch.tensor([12, 2, 7])
            h = h * len_mask(lens, L, h.dtype).unsqueeze(1)
            return dict(params=[], names=[], xs=[h], cots=[rn(B, C) if on else None for on in c['cots']], lens=lens)
        B, T = 4, 6
        return dict(params=[], names=[], xs=[rn(B, T)], cots=[rn(B)], nframes=torch.tensor([6, 1, 4, 3]) if c['nframes'] else None)

    def build(self, c, params, dev, vals):
        from audiogan_amd import ops, extras, losses
        op = c['op']
        if op == 'buildzc':
            return (lambda z, cc: (ops.BuildZCFn.apply(z, cc),)), None
        if op == 'critic_input':
            def apply(x):
                xo, lens = ops.CriticInputFn.apply(x, vals['noise'].to(dev), vals['length'].to(dev), vals['prods'])
                return xo, lens.float()
            return apply, None
        if op == 'bce':
            tg = vals['target'].to(dev) if torch.is_tensor(vals['target']) else vals['target']
            nf = vals['nframes'].to(dev) if vals['nframes'] is not None else None
            return (lambda x: ops.BCEFn.apply(x.t() if c['view'] == 't' else x, tg, nf, None)), None
        if op == 'moments':
            return (lambda h: extras._TimeMomentsFn.apply(h, vals['lens'].to(dev))), None
        nf = vals['nframes'].to(dev) if vals['nframes'] is not None else None
        return (lambda x: (losses._PerSample.apply(x, 0.5, nf),)), None

    @staticmethod
    def _bce(x, tg):
        return x.clamp(min=0) - x * tg + torch.log1p(torch.exp(-x.abs()))

    def ref(self, c, p, xs, vals):
        op = c['op']
        if op == 'buildzc':
            z, cc = xs
            return (torch.cat([z, cc.unsqueeze(1).expand(z.size(0), z.size(1), cc.size(1))], 2).transpose(0, 1),)
        if op == 'critic_input':
            ln = vals['length']
            return (xs[0] + vals['noise'].double(), torch.stack([(ln + d - 1) // d for d in vals['prods']]).double())
        if op == 'bce':
            x = xs[0].t() if c['view'] == 't' else xs[0]
            B, T = x.shape
            n = vals['nframes'] if vals['nframes'] is not None else torch.full((B,), T)
            tg = vals['target'].double().view(B, 1) if torch.is_tensor(vals['target']) else vals['target']
            per = (self._bce(x, tg) * len_mask(n, T, x.dtype)).sum(1)
            return ((per / n.double()).sum() / B, per)
        if op == 'moments':
            h, lens = xs[0], vals['lens']
            B, C, L = h.shape
            lf = lens.view(B, 1).double()
            m = h.sum(2) / lf
            cen = h - m.unsqueeze(2) * len_mask(lens, L, h.dtype).unsqueeze(1)
            return (m, (cen ** 2).sum(2) ** 0.5 / lf, (cen ** 4).sum(2) ** 0.25 / lf)
        x = xs[0]
        B, T = x.shape
        n = vals['nframes'] if vals['nframes'] is not None else torch.full((B,), T)
        return ((self._bce(x, 0.5) * len_mask(n, T, x.dtype)).sum(1),)


# ---- 6. ConvChainFn / LinearFn over a PlainGroup ---------------------------------------------------------------------
class ChainFam(Family):
    """x [B,1,L] -> two conv layers (a Conv1d / a ConvTranspose1d pair, LeakyReLU and tanh) -> mean over time -> LinearFn"""
    name = 'chain'
    routes = tuple(r for r in ROUTES if not ROUTE[r]['scope'])    # (no WNGroup: nothing is deferred to a scope)

    def cases(self):
        t = [dict(kind='conv', B=3, L=24, layers=[(4, 5, 2, 2, 0), (6, 5, 2, 2, 0)], nout=1),
             dict(kind='convT', B=2, L=6, layers=[(4, 5, 2, 2, 1), (1, 1, 1, 0, 0)], nout=3)]
        for n, c in enumerate(t):
            c.update(n=n, id='chain%d' % n)
        return t

    def classes(self, c):
        return {('kind', c['kind']), ('layers', len(c['layers']))}

    REQUIRED = {('kind', 'conv'), ('kind', 'convT'), ('layers', 2)}

    def values(self, c, seed):
        gen = _gen(seed)
        rn = lambda *s: torch.randn(*s, generator=gen)        # noqa: E731
        params, names, cin = [], [], 1
        for i, (co, k, st, pd, op) in enumerate(c['layers']):
            tr = c['kind'] == 'convT' and i == 0
            params += [rn(*((cin, co, k) if tr else (co, cin, k))) / (cin * k) ** 0.5, rn(co) * 0.2]
            names += ['l%d.w' % i, 'l%d.b' % i]
            cin = co
        params += [rn(c['nout'], cin) / cin ** 0.5, rn(c['nout']) * 0.2]
        names += ['lin.w', 'lin.b']
        B, L = c['B'], c['L']
        return dict(params=params, names=names, xs=[rn(B, 1, L)], xs2=[rn(B, 1, L)], cots=[rn(B, c['nout'])],
                    cots2=[rn(B, c['nout'])])

    def part(self, c, vals):
        return [0, 1, 2, 3]            # the conv chain frozen, the Linear trains

    def build(self, c, params, dev, vals):
        from audiogan_amd import convnets as CN, ops, kernels as K
        layers, cin = [], 1
        for i, (co, k, st, pd, op) in enumerate(c['layers']):
            tr = c['kind'] == 'convT' and i == 0
            layers.append((ops.ConvSpec('convT' if tr else 'conv', cin, co, k, st, pd, out_pad=op),
                           K.ACT_LEAKY if i == 0 else K.ACT_TANH))
            cin = co
        chain = CN.ConvChain(layers)
        for i, (sp, _) in enumerate(layers):
            chain.group.add(params[2 * i], params[2 * i + 1], sp.stride)

        def apply(x):
            a = CN.ConvChainFn.apply(x, chain, *chain.group.params())
            return (CN.LinearFn.apply(a.mean(2), params[-2], params[-1]),)
        return apply, chain.group

    def ref(self, c, p, xs, vals):
        a = xs[0]
        for i, (co, k, st, pd, op) in enumerate(c['layers']):
            if c['kind'] == 'convT' and i == 0:
                a = F.conv_transpose1d(a, p[2 * i], p[2 * i + 1], st, pd, output_padding=op)
            else:
                a = F.conv1d(a, p[2 * i], p[2 * i + 1], st, pd)
            a = leaky(a) if i == 0 else torch.tanh(a)
        return (a.mean(2) @ p[-2].t() + p[-1],)


FAMILIES = collections.OrderedDict((f.name, f) for f in (GTrunkFam(), DConvStackFam(), DHeadFam(), LSTMFam(), SmallFam(), ChainFam()))


def assert_coverage(name, cases=None):
    """the family's table meets every structural class it must (so a table edit cannot quietly drop one)"""
    fam = FAMILIES[name]
    cases = fam.cases() if cases is None else cases
    met = set()
    for c in cases:
        met |= fam.classes(c)
    missing = fam.REQUIRED - met
    assert not missing, ('block fuzz: the %s table no longer holds' % name, sorted(map(str, missing)))
    return met


# ---------------------------------------------------------------------------------------------------------------------
# runner
# ---------------------------------------------------------------------------------------------------------------------
def _cpu(t):
    return None if t is None else t.detach().cpu().clone()


def run_block(fam, case, route, dev):
    """one forward + backward of the case's Function under `route` on `dev` (whatever audiogan_amd.kernels is at the moment:
    the HIP kernels, or the CPU model).  Returns dict(outs, dxs, grads) of CPU tensors; a parameter without .grad: None"""
    from audiogan_amd import common
    vals = values(fam, case)
    LAST['bases'] = []
    params = [torch.nn.Parameter(v.to(dev).clone()) for v in vals['params']]
    apply, group = fam.build(case, params, dev, vals)
    rt = ROUTE[route]
    if rt['start'] == 'zero':
        for p in params:
            p.grad = torch.zeros_like(p.data)
    elif rt['start'] == 'rand':
        for p, s in zip(params, vals['starts']):
            p.grad = s.to(dev).clone()
    elif rt['start'] == 'some':         # .grad on the first half of the parameters only (an LSTM layer: on direction 0 only)
        for p in params[:fam.some(case, vals)]:
            p.grad = torch.zeros_like(p.data)
    elif rt['start'] == 'nc':
        for p in params:
            p.grad = _nc_like(p.data)
            assert p.numel() == 1 or common.grad_target(p) is None

    def inputs(which):
        xs = [fam.place(case, i, v, dev) for i, v in enumerate(vals[which])]
        for x, r in zip(xs, vals['req']):
            x.requires_grad_(bool(r) and not rt['nox'])
        return xs
    xs = inputs('xs')
    xs2 = inputs('xs2') if rt['twice'] else None
    if rt['freeze'] == 'all':
        ctx = common.frozen(params)
    elif rt['freeze'] == 'part':
        ctx = common.frozen([params[i] for i in fam.part(case, vals)])
    else:
        ctx = contextlib.nullcontext()
    import audiogan_amd.kernels as K
    prec = contextlib.nullcontext() if is_f32(case) else K.precision('bf16')
    with prec:
        got = _run_routes(fam, case, route, dev, vals, params, apply, xs, xs2, ctx)
    fam.after_run(case, route)
    return got


def _run_routes(fam, case, route, dev, vals, params, apply, xs, xs2, ctx):
    from audiogan_amd import common
    rt = ROUTE[route]
    with (ctx if rt['when'] == 'fwd' else contextlib.nullcontext()):
        outs = apply(*xs)
        outs2 = apply(*xs2) if xs2 is not None else None
    ts, gs = [], []
    for oo, cc in ((outs, vals['cots']),) + (((outs2, vals['cots2']),) if outs2 is not None else ()):
        for j, (o, ct) in enumerate(zip(oo, cc)):
            if ct is not None and o.requires_grad:
                ts.append(o)
                gs.append(fam.cot(case, j, ct, dev))
    if ts:
        with (ctx if rt['when'] == 'bwd' else contextlib.nullcontext()), \
                (common.network_backward() if rt['scope'] else contextlib.nullcontext()), warnings.catch_warnings():
            warnings.simplefilter('ignore', UserWarning)        # ('noncontig': torch remarks on the layout of such a .grad)
            torch.autograd.backward(ts, gs)
    if torch.device(dev).type == 'cuda':
        torch.cuda.synchronize()
    return dict(outs=[_cpu(o) for o in outs], dxs=[_cpu(x.grad) for x in xs],
                dxs2=[_cpu(x.grad) for x in xs2] if xs2 is not None else None, grads=[_cpu(p.grad) for p in params])


_REFS = {}


def ref_block(fam, case, route):
    """the float64 reference of what run_block returns for this route (computed once per case: the routes differ only in
    how the same gradients are delivered)"""
    vals = values(fam, case)
    key = (fam.name, case['id'])
    if key not in _REFS:
        res = []
        for which, cw in (('xs', 'cots'), ('xs2', 'cots2')):
            p = [v.double().requires_grad_(True) for v in vals['params']]
            xs = [v.double().requires_grad_(True) for v in vals[which]]
            outs = fam.ref(case, p, xs, vals)
            assert len(outs) == len(vals[cw])
            loss = sum((o * ct.double()).sum() for o, ct in zip(outs, vals[cw]) if ct is not None)
            g = torch.autograd.grad(loss, p + xs, allow_unused=True)
            g = [torch.zeros_like(t) if gi is None else gi for gi, t in zip(g, p + xs)]
            res.append(dict(outs=[o.detach() for o in outs], gp=g[:len(p)], gx=g[len(p):]))
        _REFS[key] = res
    a, b = _REFS[key]
    n = len(vals['params'])
    rt = ROUTE[route]
    gp = [x + y for x, y in zip(a['gp'], b['gp'])] if rt['twice'] else a['gp']
    froz = set(range(n)) if rt['freeze'] == 'all' else set(fam.part(case, vals)) if rt['freeze'] == 'part' else set()
    start = {'rand': [s.double() for s in vals['starts']], 'zero': [torch.zeros_like(g) for g in gp]}.get(rt['start'])
    if start is not None:       # a frozen parameter keeps its start, the others hold start + gradient
        gp = [s if i in froz else s + g for i, (s, g) in enumerate(zip(start, gp))]
    else:
        gp = [None if i in froz else g for i, g in enumerate(gp)]
    if not any(ct is not None for ct in vals['cots']):
        gp = [None] * n
    req = [bool(r) and not rt['nox'] for r in vals['req']]
    return dict(outs=a['outs'], dxs=[g if r else None for g, r in zip(a['gx'], req)],
                dxs2=[g if r else None for g, r in zip(b['gx'], req)] if rt['twice'] else None, grads=gp,
                gp_plain=a['gp'])


def _entries(fam, case, got, ref):
    vals = values(fam, case)
    out = []
    for j, (g, r) in enumerate(zip(got['outs'], ref['outs'])):
        out.append(('out%d' % j, g, r, None))
    for key in ('dxs', 'dxs2'):
        if ref[key] is not None:
            for j, (g, r) in enumerate(zip(got[key], ref[key])):
                out.append(('%s%d' % (key[:-1], j), g, r, None))
    for i, (g, r) in enumerate(zip(got['grads'], ref['grads'])):
        extra = None
        if i in vals['bias_v'] and r is not None:
            # the v-gradient of a bias is identically 0 (w = g sign(v)); its error is a fraction of |g / v| |dL/dg|, the
            # size of the two terms that cancel
            v, gg = vals['params'][i].double(), vals['params'][vals['bias_v'][i]].double()
            extra = float(((gg / v).abs() * ref['gp_plain'][vals['bias_v'][i]].abs()).max())
        out.append(('d.' + vals['names'][i], g, r, extra))
    return out


def errors(fam, case, got, ref):
    """name -> (error as a fraction of the scale, scale); structural checks (None-ness, shapes, finiteness) on the way"""
    res = {}
    tag = (case['id'],)
    for name, g, r, extra in _entries(fam, case, got, ref):
        if r is None:
            assert g is None, ('a gradient where none is due: ' + name,) + tag
            continue
        assert g is not None, ('no gradient: ' + name,) + tag
        assert tuple(g.shape) == tuple(r.shape), ('shape: ' + name,) + tag + (tuple(g.shape), tuple(r.shape))
        assert bool(torch.isfinite(g.float()).all()), ('not finite: ' + name,) + tag
        scale = max(float(r.abs().max()), extra or 0.0)
        d = float((g.double() - r).abs().max())
        if scale == 0.0:
            assert d == 0.0, ('out of bound: ' + name + ' (the reference is exactly 0)',) + tag + (d,)
            continue
        res[name] = (d / scale, scale)
    return res


def check_block(fam, case, route, got, ref, floor, again=None):
    """got against float64 under the bound rule; `floor`: what ``errors`` gave for the CPU model's run of the same case and
    route.  Returns name -> error / floor."""
    if again is not None:
        for k in ('outs', 'dxs', 'dxs2', 'grads'):
            assert same_bits(got[k], again[k]), ('not reproducible: ' + k, case['id'], route)
    if not is_f32(case):
        return check_block_bf16(fam, case, route, got, ref)
    margin = margin_of(fam.name)
    ratios = {}
    LAST['detail'] = {}
    for name, (e, scale) in errors(fam, case, got, ref).items():
        f = max(floor[name][0] if name in floor else 0.0, FLOOR_MIN)
        ratios[name] = e / f
        LAST['detail'][name] = (e, f)
        assert e <= bound(margin, f), ('out of bound: ' + name, case['id'], route, 'error / floor %.2f' % (e / f), e)
    return ratios


def check_block_bf16(fam, case, route, got, ref):
    """a bf16-precision / bf16-storage case against the float64 block with rounded contractions (contract_of): the declared
    tolerances of tests/test_bf16.py.  Returns name -> error / tolerance (the larger of elementwise and L2)"""
    vals = values(fam, case)
    store = contract_of(case).mode == 'store'
    ratios = {}
    if route == 'fresh':
        # the mode is really on: the output is more than 10 times further from the unrounded float64 block
        c32 = dict(case, mode='f32', id=case['id'] + ' unrounded')
        _VALS[(fam.name, c32['id'])] = vals
        o16, o32, o = ref['outs'][0], ref_block(fam, c32, 'fresh')['outs'][0], got['outs'][0].double()
        assert float((o - o32).norm()) > 10 * float((o - o16).norm()), ('did not round: out0', case['id'])
    for name, g, r, extra in _entries(fam, case, got, ref):
        if r is None:
            assert g is None, ('a gradient where none is due: ' + name, case['id'])
            continue
        assert g is not None and tuple(g.shape) == tuple(r.shape), ('no gradient / shape: ' + name, case['id'])
        assert bool(torch.isfinite(g.float()).all()), ('not finite: ' + name, case['id'])
        if extra is not None:
            continue                    # the v-gradient of a bias
        par = name.startswith('d.')
        if par and ROUTE[route]['start'] == 'rand':
            i = vals['names'].index(name[2:])
            g, r = g.double() - vals['starts'][i].double(), r - vals['starts'][i].double()     # the gradient without its start
        scale = float(r.abs().max())
        d = (g.double() - r).abs()
        if scale == 0.0:
            assert float(d.max()) <= (1e-6 if ROUTE[route]['start'] == 'rand' and ROUTE[route]['freeze'] is None else 0.0), \
                ('out of bound: ' + name, case['id'], route)
            continue
        elem = (BF16_PAR['elem_store' if store else 'elem']) if par else BF16_ACT['elem']
        l2 = (BF16_PAR['l2_gain' if name.endswith('_g') else 'l2']) if par else BF16_ACT['l2_store' if store else 'l2']
        e_elem, e_l2 = float(d.max()) / scale, float((g.double() - r).norm() / r.norm())
        ratios[name] = max(e_elem / elem, e_l2 / l2)
        assert e_elem <= elem and e_l2 <= l2, ('out of bound: ' + name, case['id'], route, 'elementwise %.2e (%.0e)  L2 %.2e (%.0e)'
                                              % (e_elem, elem, e_l2, l2))
    return ratios


def check_routes(fam, case, got):
    """the bit equalities between routes the project claims: deferral and direct accumulation change no bit"""
    fresh = got['fresh']
    tag = (case['id'],)
    for r in SAME_AS_FRESH:
        if r not in got:
            continue
        for i, (a, b) in enumerate(zip(got[r]['grads'], fresh['grads'])):
            assert same_value_bits(a, b), ('route changes bits: %s vs fresh, parameter %d' % (r, i),) + tag
        assert same_bits(got[r]['outs'], fresh['outs']), ('route changes the forward: ' + r,) + tag
        if r != 'nograd_x':
            assert same_bits(got[r]['dxs'], fresh['dxs']), ('route changes dx: ' + r,) + tag
    if 'frozen' in got:
        vals = values(fam, case)
        for i, (a, s) in enumerate(zip(got['frozen']['grads'], vals['starts'])):
            assert same_bits(a, s), ('frozen: .grad touched, parameter %d' % i,) + tag
        assert same_bits(got['frozen']['dxs'], fresh['dxs']), ('frozen: dx differs from fresh',) + tag
    for r in [r for r in PART_ROUTES if r in got]:
        # partly frozen, at forward time or during the backward: a frozen parameter's .grad is bit-unchanged (none appears
        # where none was), the others hold what the fresh route gives (from a zero start: its bits), dx has fresh's bits
        vals, start = values(fam, case), ROUTE[r]['start']
        froz = set(fam.part(case, vals))
        for i, (a, b) in enumerate(zip(got[r]['grads'], fresh['grads'])):
            if i in froz:
                want = dict(rand=vals['starts'][i], zero=torch.zeros_like(vals['starts'][i])).get(start)
                assert same_bits(a, want), ('partly frozen (%s): .grad touched, parameter %d' % (r, i),) + tag
            elif start != 'rand':
                assert same_value_bits(a, b), ('partly frozen (%s): parameter %d differs from fresh' % (r, i),) + tag
        assert same_bits(got[r]['dxs'], fresh['dxs']), ('partly frozen (%s): dx differs from fresh' % r,) + tag


def run_case(fam, case, dev, routes=None, after=None, twice=True):
    """every route of a case -> {route: got}; '<route>_again' is the second run for the determinism check (the routes whose
    bits are not tied to another route's anyway)"""
    got = {}
    for r in (routes or fam.routes):
        got[r] = run_block(fam, case, r, dev)
        if after is not None:
            after(case, r)
        if twice and r in RUN_TWICE:
            got[r + '_again'] = run_block(fam, case, r, dev)
            if after is not None:
                after(case, r)
    return got


def floors(fam, cases=None):
    """{(case id, route): errors of the CPU model's run}  -  call it with the kernel model installed"""
    import audiogan_amd.kernels as K
    assert K.gemm.__module__ == 'tests.kernel_model', 'the floor is the error of the CPU kernel model'
    out = {}
    for case in (fam.cases() if cases is None else cases):
        for r in fam.routes:       # (a bf16 case has no floor: its tolerance is declared)
            out[(case['id'], r)] = errors(fam, case, run_block(fam, case, r, 'cpu'), ref_block(fam, case, r)) if is_f32(case) else {}
    return out


def sweep(fam, dev, floor, worst=None, after=None, cases=None, expect=None):
    """every case under every route: float64 bounds, route bit equalities, determinism.  `expect(case)`: per-case branch
    assertions of the caller (a context manager around the case's runs)"""
    worst = {} if worst is None else worst
    if cases is None:       # (the CPU kernel model has neither precision modes nor bf16 storage)
        cases = fam.cases() if torch.device(dev).type == 'cuda' else host_cases(fam)
    for case in cases:
        with (expect(case) if expect is not None else contextlib.nullcontext()):
            got = run_case(fam, case, dev, after=after)
        for r in fam.routes:
            ratios = check_block(fam, case, r, got[r], ref_block(fam, case, r), floor[(case['id'], r)],
                                 again=got.get(r + '_again'))
            tag = fam.name if is_f32(case) else '%s %s (/ tolerance)' % (fam.name, case['mode'])
            for k, v in ratios.items():
                merge_worst(worst, tag, {'dparam' if k.startswith('d.') else k: v})
            merge_worst(worst, tag + ' route ' + r, {'max': max(ratios.values()) if ratios else 0.0})
            if ratios and is_f32(case):
                k = max(ratios, key=ratios.get)
                if ratios[k] > max(worst.get(tag + ' largest', {'': 0.0}).values()):
                    worst[tag + ' largest'] = {'%s %s %s error %.1e floor %.1e ratio' % ((case['id'], r, k) + LAST['detail'][k]): ratios[k]}
        check_routes(fam, case, got)
    return worst


# ---------------------------------------------------------------------------------------------------------------------
# weight caches
# ---------------------------------------------------------------------------------------------------------------------
def run_cache(fam, case, dev, how):
    """forward, change a parameter (`how`: 'inplace' - an in-place op under no_grad; 'optim' - one optimiser step, a
    raw-pointer write plus bump_param_epoch), forward again.  Returns (second outputs, the parameters as they are now)"""
    from audiogan_amd import optim
    vals = values(fam, case)
    params = [torch.nn.Parameter(v.to(dev).clone()) for v in vals['params']]
    apply, group = fam.build(case, params, dev, vals)
    import audiogan_amd.kernels as K
    with (contextlib.nullcontext() if is_f32(case) else K.precision('bf16')):
        return _run_cache(fam, case, dev, how, vals, params, apply)


def _run_cache(fam, case, dev, how, vals, params, apply):
    from audiogan_amd import optim
    xs = [fam.place(case, i, v, dev) for i, v in enumerate(vals['xs'])]
    first = apply(*xs)
    if how == 'inplace':
        with torch.no_grad():
            for p in params:
                p.mul_(1.25)
    else:
        for p, s in zip(params, vals['starts']):
            p.grad = s.to(dev).clone()
        optim.RMSprop(params, lr=0.05).step()
    outs = apply(*[fam.place(case, i, v, dev) for i, v in enumerate(vals['xs'])])
    now = [_cpu(p.data) for p in params]
    assert not all(same_bits(a, b) for a, b in zip(now, vals['params'])), 'the parameters did not change'
    del first
    return [_cpu(o) for o in outs], now


def cache_errors(fam, case, outs, now):
    vals = values(fam, case)
    ref = fam.ref(case, [p.double() for p in now], [x.double() for x in vals['xs']], vals)
    res = {}
    for j, (g, r) in enumerate(zip(outs, ref)):
        scale = float(r.abs().max())
        res['out%d' % j] = (float((g.double() - r).abs().max()) / scale, scale, float((g.double() - r).norm() / r.norm()))
    return res


def check_cache(fam, case, dev, floor):
    """the second forward is held to float64 ON THE NEW PARAMETERS; `floor`: {how: cache_errors of the CPU model}"""
    ratios = {}
    for how in ('inplace', 'optim'):
        outs, now = run_cache(fam, case, dev, how)
        for name, (e, _, l2) in cache_errors(fam, case, outs, now).items():
            if not is_f32(case):        # the declared bf16 tolerances (a stale bf16 image is off by the 25 % the weights moved)
                store = contract_of(case).mode == 'store'
                ratios['%s.%s' % (how, name)] = max(e / BF16_ACT['elem'], l2 / BF16_ACT['l2_store' if store else 'l2'])
                assert ratios['%s.%s' % (how, name)] <= 1.0, ('stale weights after a parameter changed (%s): %s' % (how, name),
                                                              case['id'], e, l2)
                continue
            f = max(floor[how][name][0], FLOOR_MIN)
            ratios['%s.%s' % (how, name)] = e / f
            assert e <= bound(margin_of(fam.name), f), ('stale weights after a parameter changed (%s): %s' % (how, name),
                                                      case['id'], e / f)
    return ratios


def cache_floors(fam, case):
    if not is_f32(case):
        return None
    return {how: cache_errors(fam, case, *run_cache(fam, case, 'cpu', how)) for how in ('inplace', 'optim')}


def check_changed_between(fam, case, dev):
    """a parameter changed between forward and backward raises the Functions' own assertion"""
    vals = values(fam, case)
    params = [torch.nn.Parameter(v.to(dev).clone()) for v in vals['params']]
    apply, group = fam.build(case, params, dev, vals)
    xs = [fam.place(case, i, v, dev).requires_grad_(True) for i, v in enumerate(vals['xs'])]
    outs = apply(*xs)
    with torch.no_grad():
        params[0].mul_(1.25)
    try:
        torch.autograd.backward([o for o, ct in zip(outs, vals['cots']) if ct is not None],
                                [ct.to(dev) for ct in vals['cots'] if ct is not None])
    except AssertionError as e:
        assert 'parameters changed between forward and backward' in str(e)
        return
    raise AssertionError(('a parameter changed between forward and backward went unnoticed', case['id']))


# family -> indices of its weight-cache cases (dhead 10: the bf16 images of WNGroup.w16; lstm 13: common.Bf16Images)
CACHE_CASES = dict(gtrunk=[1], dconv=[4], dhead=[4, 10], lstm=[13], chain=[0])


def bce_backward_without_gradient():
    """ops.BCEFn.backward with ``dloss is None`` (the loss took no gradient): four Nones and no launch"""
    from audiogan_amd import ops
    e = torch.empty(0)
    assert ops.BCEFn.backward(types.SimpleNamespace(saved_tensors=(torch.zeros(2, 3), e, e)), None, None) == (None,) * 4


def host_cases(fam):
    """the cases the CPU kernel model can run (it has neither precision modes nor bf16 storage)"""
    return [c for c in fam.cases() if is_f32(c)]
