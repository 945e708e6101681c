"""Shared pieces of the deferred-reduction sequence fuzz (test_reduce_fuzz.py on the GPU, test_reduce_fuzz_host.py here)
--  TEST INFRASTRUCTURE, no test functions.

The five launch fuzzes pin one call at a time.  This one pins what happens ACROSS reducing calls inside one
``kernels.deferred_reduces`` scope: the table of 40 recorded second stages of csrc/api.hip, the one launch that sums them, the
clash rule and the order of writes into one destination.

  Seq                   a SEQUENCE: frames, destinations and a list of items.  An item is a Step - one reducing call through
                        audiogan_amd.kernels with a destination name - or one of ('inner+',) / ('inner-',) (open / close an
                        inner ``deferred_reduces()`` block of an ``outer=True`` scope), ('flush',) (``flush_reduces()``) and
                        ('check', name) (a named checkpoint: synchronize and look at every destination).
                        A destination is a window ([rows, ncol] of row pitch ld) in a sentinel frame of conv_cases (FlatFrame /
                        StridedFrame), NaN-filled when its first writer does not accumulate and at a known non-zero start when
                        it does; what a frame holds beside its destinations is a third filler that must come back unchanged.
                        Inputs sit in frames filled with 99.
  stage makers          col_sum / channel_sum / conv_wgrad / gemm(ta=True) / gemm_h(ta=True), each at the smallest shape that
                        takes its branch: `two_stage()` restates which form a call takes (single writer, or partial sums + a
                        second stage), `slabs()` how many partial sums it leaves, `vec_stage()` which descriptor it records.
  trace() / model()     a pure-Python model of the recording rules, restated from the contract in csrc/api.hip and the
                        docstring of kernels.deferred_reduces: a stage is recorded when its call is two-stage and deferral is
                        recording (an owner scope: always; an outer scope: inside an inner block) and the call does not ask
                        for ``defer=False``; the table is summed when it holds 40 stages or when the new destination's span
                        overlaps a recorded one; a direct write is final at once and sums the table first when its span
                        overlaps a recorded one; flush_reduces() and the end of the scope sum the table.  model(seq) gives,
                        after every item, the set of destinations that are final.
  passes                EXACT  integer inputs in [1, 3] - no stage sums to zero, so a pending destination can be told from a
                               final one - and non-zero integer starts; 9 x (reduction length) < 2^24 (asserted), so every
                               order of summation is exact and the result equals the float64 reference BIT FOR BIT.
                        REAL   randn inputs scaled by (reduction length)^-1/2, non-zero real starts; the bound rule of
                               DESIGN.md section 2 as pointwise_cases applies it to col_sum: floor = the error of the same
                               arithmetic in fp32 on the CPU against float64, as a fraction of the reference's largest
                               magnitude, not below 2^-24; bound = margin x floor, never above 1e-4.
  reference()           float64 (or fp32: the floor), restating each call's contract; it does not call tests/kernel_model.py.
  run() / check_seq()   run a sequence plain (no scope) and scoped, twice; assert what the module docstring of
                        test_reduce_fuzz.py lists.
  coverage()            every class the sequence lists must reach, so that none can drop out.
"""
import collections

import torch
import torch.nn.functional as F

from tests import conv_cases as CC

EXACT, REAL = CC.EXACT, CC.REAL
SLAB_MAXD = 40             # csrc/api.hip
SMALL_WS = 1 << 17         # kernels._SMALL_WS
REST = 555.0               # what a frame holds beside its destinations
MARGIN = CC.MARGIN
# kernel label -> a margin above 16 with its measured ratio and reason.  None is needed: profiles/reduce_fuzz.txt
MARGINS = {}

Step = collections.namedtuple('Step', 'kind dest acc defer p')
Dest = collections.namedtuple('Dest', 'frame off rows ncol ld')     # off: floats from the frame window's first float

cdiv = CC.cdiv


# ---------------------------------------------------------------------------------------------------------------------
# the forms of a call, restated on sizes alone
# ---------------------------------------------------------------------------------------------------------------------
def two_stage(s):
    """does this call leave partial sums and a second stage (True), or write its output as the single writer (False)?"""
    p = s.p
    if s.kind == 'col_sum':            # ag_col_sum: gy = min(ceil(1024 / gx), ceil(M / 16)) row blocks, one -> single writer
        return slabs(s) > 1
    if s.kind == 'channel_sum':        # ag_channel_sum: nsplit = ceil(B L / 4096), at most ceil(2048 / C)
        return slabs(s) > 1
    if s.kind == 'conv_wgrad':         # always
        return True
    assert s.kind in ('gemm', 'gemm_h') and p['M'] <= 64 and p['N'] <= 64
    return p['K'] >= 1024              # one output tile: K >= 1024 is split (4 slices at K = 1024)


def slabs(s):
    p = s.p
    if s.kind == 'col_sum':
        assert p['N'] <= 64
        gy = max(1, min(1024, cdiv(p['M'], 16)))
        ws = min(SMALL_WS, 64 * p['N']) if p['M'] > 16 else 0
        gy = min(gy, ws // p['N']) if gy > 1 and ws >= 2 * p['N'] else 1
        return cdiv(p['M'], cdiv(p['M'], gy))
    if s.kind == 'channel_sum':
        return max(1, min(cdiv(p['B'] * p['L'], 4096), cdiv(2048, p['C'])))
    if s.kind in ('gemm', 'gemm_h'):
        if p['K'] < 1024:
            return 1
        ks = [c for c in (32, 24, 16, 8, 4, 2) if c <= (512 * 4 + 2) // 3 and c <= p['K'] // 256][0]
        return cdiv(p['K'], CC.roundup(cdiv(p['K'], ks), 64))
    return None                        # conv_wgrad: the slices of its grid (tests/conv_cases.py restates them)


def red_len(s):
    p = s.p
    return dict(col_sum=lambda: p['M'], channel_sum=lambda: p['B'] * p['L'], conv_wgrad=lambda: p['B'] * p['Lsh'],
                gemm=lambda: p['K'], gemm_h=lambda: p['K'])[s.kind]()


def label(s, d):
    form = 'two-stage' if two_stage(s) else 'direct'
    pitch = '' if s.kind not in ('gemm', 'gemm_h') else (' contiguous' if d.ld == d.ncol else ' pitched')
    return '%s %s%s' % (s.kind, form, pitch)


# ---------------------------------------------------------------------------------------------------------------------
# sequences
# ---------------------------------------------------------------------------------------------------------------------
class Seq(object):
    def __init__(self, name, cls, outer=False, stream=False):
        self.name, self.cls, self.outer, self.stream = name, cls, outer, stream
        self.frames = collections.OrderedDict()      # name -> ('flat', n) | ('mat', rows, width, ld, off)
        self.dests = collections.OrderedDict()       # name -> Dest
        self.items = []
        self.tags = set([cls])                       # coverage classes this sequence declares

    # frames and destinations
    def flat(self, name, n, rows=1):
        """a contiguous destination [rows, n / rows] that is a frame of its own"""
        self.frames[name] = ('flat', n)
        self.dests[name] = Dest(name, 0, rows, n // rows, n // rows)
        return name

    def frame(self, name, *geo):
        self.frames[name] = geo

    def dest(self, name, frame, off, rows, ncol, ld=None):
        self.dests[name] = Dest(frame, off, rows, ncol, ncol if ld is None else ld)
        return name

    def block(self, name, rows, ncol, ld, off=0):
        """a [rows, ncol] column block of a [rows, ld - 1 or so] matrix of row pitch ld, a frame of its own"""
        self.frames[name] = ('mat', rows, ncol, ld, off)
        self.dests[name] = Dest(name, 0, rows, ncol, ld)
        return name

    # items
    def step(self, kind, dest, acc=1, defer=True, **p):
        s = Step(kind, dest, int(acc), bool(defer), p)
        d = self.dests[dest]
        n = d.rows * d.ncol
        want = dict(col_sum=lambda: (1, p['N']), channel_sum=lambda: (1, p['C']),
                    conv_wgrad=lambda: (1, p['A'] * p['C'] * 3), gemm=lambda: (p['M'], p['N']),
                    gemm_h=lambda: (p['M'], p['N']))[kind]()
        assert (d.rows, d.ncol) == want and n > 0, (self.name, s, d)
        assert kind != 'conv_wgrad' or acc == 1
        assert 9 * red_len(s) < 2 ** 24
        self.items.append(s)
        return s

    def mark(self, *item):
        self.items.append(tuple(item))

    def steps(self):
        return [(i, it) for i, it in enumerate(self.items) if isinstance(it, Step)]

    def first_acc(self, dest):
        return [s.acc for _, s in self.steps() if s.dest == dest][0]

    def base_off(self, d):
        g = self.frames[d.frame]
        return (g[4] if g[0] == 'mat' else 0) + d.off


def span(d):
    return (d.rows - 1) * d.ld + d.ncol


def overlap(a, b):
    """the clash rule of slab_record: spans compared whole"""
    return a.frame == b.frame and a.off < b.off + span(b) and b.off < a.off + span(a)


def vec_stage(seq, s):
    """the descriptor a recorded stage gets: float4 outputs when n, ncol, ld % 4 == 0 and the destination is 16-byte aligned
    (the workspaces are)"""
    d = seq.dests[s.dest]
    return (d.rows * d.ncol) % 4 == 0 and d.ncol % 4 == 0 and d.ld % 4 == 0 and seq.base_off(d) % 4 == 0


# stage makers: one new destination and one step each, at the smallest shape that takes the branch
def st_col(seq, name, Z=2, N=8, acc=1, defer=True):
    """Z >= 2: M = 16 Z rows give exactly Z slabs (rows_per = 16); Z = 0: the direct form, M = 8"""
    seq.flat(name, N)
    return seq.step('col_sum', name, acc, defer, M=16 * Z if Z else 8, N=N)


def st_chan(seq, name, C=5, two=True, acc=1):
    seq.flat(name, C)
    return seq.step('channel_sum', name, acc, True, B=2, C=C, L=2050 if two else 32)


def st_conv(seq, name, vec=True):
    A, C = (4, 2) if vec else (3, 3)
    seq.flat(name, A * C * 3)
    return seq.step('conv_wgrad', name, 1, True, B=1, A=A, C=C, Lsh=8)


def st_gemm(seq, name, form='c', two=True, acc=1, defer=True, kind='gemm'):
    """form: 'c' contiguous, 'pv' a column block with ld != ncol, both % 4 == 0, 'ps' a column block with odd ncol and ld"""
    M, N, ld, off = dict(c=(8, 8, 8, 0), pv=(8, 8, 16, 4), ps=(8, 7, 17, 3))[form]
    if kind == 'gemm_h':
        N = 8                                       # (bf16 operands: row counts % 8 == 0; the pitch still makes it scalar)
    if form == 'c':
        seq.flat(name, M * N, rows=M)
    else:
        seq.block(name, M, N, ld, off)
    return seq.step(kind, name, acc, defer, M=M, N=N, K=1024 if two else 512)


CYCLE = ('col vec', 'col scalar', 'conv vec', 'conv scalar', 'gemm c', 'gemm ps', 'gemm pv', 'chan scalar')


def st_cycle(seq, name, k, acc=1):
    """stage kinds in a fixed cycle that alternates vector and scalar descriptors (a conv weight gradient always accumulates)"""
    what = CYCLE[k % len(CYCLE)]
    if what == 'col vec':
        return st_col(seq, name, 2 + k % 3, 8, acc)
    if what == 'col scalar':
        return st_col(seq, name, 2 + k % 3, 7, acc)
    if what == 'conv vec':
        return st_conv(seq, name, True)
    if what == 'conv scalar':
        return st_conv(seq, name, False)
    if what == 'chan scalar':
        return st_chan(seq, name, 5, True, acc)
    return st_gemm(seq, name, what.split()[1], True, acc)


Z_SWEEP = (2, 7, 8, 9, 24, 25, 32, 33, 56, 57, 64)
TABLE_SIZES = (1, 2, 39, 40, 41, 80, 81)
ACC_PAIRS = ((1, 1), (0, 1), (1, 0), (0, 0))


def z_sequences():
    out = []
    for Z in Z_SWEEP:
        a = Seq('z%d alone' % Z, 'z sweep')
        b = Seq('z%d last of five' % Z, 'z sweep')
        k = 0
        for N in (8, 7):
            for acc in (0, 1):
                st_col(a, 'n%d acc%d' % (N, acc), Z, N, acc)
                a.mark('flush')
                for j in range(4):
                    st_cycle(b, 'n%d acc%d fill%d' % (N, acc, j), k)
                    k += 1
                st_col(b, 'n%d acc%d' % (N, acc), Z, N, acc)
                b.mark('flush')
                for q in (a, b):
                    q.tags.add(('z', Z, 'vec' if N % 4 == 0 else 'scalar', acc, 'alone' if q is a else 'last of five'))
        out += [a, b]
    return out


def table_sequences():
    out = []
    for n in TABLE_SIZES:
        q = Seq('table %d' % n, 'table')
        for k in range(n):
            st_cycle(q, 'd%02d' % k, k + n % 2, acc=(k // 3) % 2)
            if k + 1 in (SLAB_MAXD, SLAB_MAXD + 1, 2 * SLAB_MAXD, 2 * SLAB_MAXD + 1) or k + 1 == n:
                q.mark('check', 'after %d' % (k + 1))
        q.tags.add(('table', n))
        out.append(q)
    return out


def clash_sequences():
    out = []
    for a0, a1 in ACC_PAIRS:
        q = Seq('same output acc %d/%d' % (a0, a1), 'clash')
        q.flat('out', 8)
        q.step('col_sum', 'out', a0, M=48, N=8)
        q.mark('check', 'one')
        q.step('col_sum', 'out', a1, M=32, N=8)
        q.mark('check', 'two')
        q.tags.add(('clash', 'same output', a0, a1))
        out.append(q)
    q = Seq('column blocks of one matrix', 'clash')          # dw_ih[:, :Fx] and dw_ih[:, Fx:] as recurrent.py issues them
    q.frame('dw', 'mat', 8, 20, 24, 0)
    q.dest('left', 'dw', 0, 8, 8, 24)
    q.dest('right', 'dw', 8, 8, 12, 24)
    q.step('gemm', 'left', 1, M=8, N=8, K=1024)
    q.step('gemm', 'right', 1, M=8, N=12, K=1024)
    q.mark('check', 'two')
    q.tags.add(('clash', 'column blocks'))
    out.append(q)
    q = Seq('adjacent vectors of one buffer', 'clash')
    q.frame('buf', 'flat', 15)
    q.dest('lo', 'buf', 0, 1, 8)
    q.dest('hi', 'buf', 8, 1, 7)
    q.step('col_sum', 'lo', 1, M=32, N=8)
    q.step('col_sum', 'hi', 0, M=32, N=7)
    q.mark('check', 'two')
    q.tags.add(('clash', 'adjacent'))
    out.append(q)
    q = Seq('vector inside the span of a pitched block', 'clash')
    q.frame('m', 'mat', 4, 12, 16, 0)
    q.dest('blk', 'm', 0, 4, 8, 16)
    q.dest('row', 'm', 16 + 8, 1, 4)
    q.step('gemm', 'blk', 0, M=4, N=8, K=1024)
    q.step('col_sum', 'row', 0, M=32, N=4)
    q.mark('check', 'two')
    q.tags.add(('clash', 'inside span'))
    out.append(q)
    return out


def mixed_sequences():
    """a two-stage and a direct call into ONE destination, in both orders"""
    out = []

    def pair(kind, accs, order, defer2):
        q = Seq('mixed %s acc %d/%d %s, second defer=%s' % (kind, accs[0], accs[1], order, defer2), 'mixed')
        forms = (True, False) if order == 'two-stage then direct' else (False, True)
        for j, (two, acc) in enumerate(zip(forms, accs)):
            defer = True if j == 0 else defer2
            if kind == 'col_sum':
                if j == 0:
                    q.flat('out', 8)
                q.step('col_sum', 'out', acc, defer, M=32 if two else 8, N=8)
            elif kind == 'channel_sum':
                if j == 0:
                    q.flat('out', 5)
                q.step('channel_sum', 'out', acc, True, B=2, C=5, L=2050 if two else 32)
            else:
                if j == 0:
                    q.block('out', 8, 8, 16, 4)
                q.step(kind, 'out', acc, defer, M=8, N=8, K=1024 if two else 512)
            q.mark('check', 'after %d' % (j + 1))
        q.tags.add(('mixed', kind, accs, order, defer2))
        return q

    for order in ('two-stage then direct', 'direct then two-stage'):
        for defer2 in (True, False):
            out += [pair('col_sum', (1, 1), order, defer2), pair('col_sum', (1, 0), order, defer2),
                    pair('gemm', (1, 1), order, defer2), pair('gemm_h', (1, 1), order, defer2)]
        out.append(pair('channel_sum', (1, 1), order, True))
    return out


def scope_sequences():
    out = []
    q = Seq('owner scope', 'scope')
    for k in range(5):
        st_cycle(q, 'd%d' % k, k, acc=k % 2)
    q.mark('check', 'inside')
    q.tags.add(('scope', 'owner'))
    out.append(q)

    q = Seq('outer scope, two inner blocks', 'scope', outer=True)
    st_col(q, 'before', 2, 8, 1)                     # outside every inner block: not recorded
    q.mark('inner+')
    st_cycle(q, 'a0', 0, 0)
    st_cycle(q, 'a1', 5, 1)
    q.mark('inner-')
    st_col(q, 'between', 3, 7, 1, defer=False)
    q.mark('check', 'between')
    q.mark('inner+')
    q.mark('inner+')                                 # (a Function's block inside another's)
    st_cycle(q, 'b0', 2, 1)
    q.mark('inner-')
    st_cycle(q, 'b1', 7, 0)
    q.mark('inner-')
    q.mark('check', 'before exit')
    q.tags.add(('scope', 'outer'))
    out.append(q)

    q = Seq('flush_reduces mid-scope', 'scope')
    st_cycle(q, 'a0', 1, 0)
    st_cycle(q, 'a1', 4, 1)
    q.mark('flush')
    q.mark('check', 'flushed')
    st_cycle(q, 'b0', 6, 1)
    st_cycle(q, 'b1', 0, 0)
    q.mark('check', 'recording again')
    q.tags.add(('scope', 'flush'))
    out.append(q)

    q = Seq('scope on a side stream', 'scope', stream=True)
    for k in range(6):
        st_cycle(q, 'd%d' % k, k + 3, acc=(k + 1) % 2)
    q.mark('flush')
    q.mark('check', 'flushed')
    st_col(q, 'late', 9, 8, 1)
    q.tags.add(('scope', 'side stream'))
    out.append(q)
    return out


def gemm_h_sequences():
    q = Seq('gemm_h destinations', 'gemm_h')
    for j, form in enumerate(('c', 'pv', 'ps')):
        st_gemm(q, 'two %s' % form, form, True, j % 2, kind='gemm_h')
        st_gemm(q, 'direct %s' % form, form, False, (j + 1) % 2, kind='gemm_h')
        q.tags.add(('gemm_h', form))
    q.mark('check', 'inside')
    return [q]


def all_sequences():
    return z_sequences() + table_sequences() + clash_sequences() + mixed_sequences() + scope_sequences() + gemm_h_sequences()


# ---------------------------------------------------------------------------------------------------------------------
# the model of the recording rules
# ---------------------------------------------------------------------------------------------------------------------
def trace(seq, flush_before_direct=True):
    """one record per item, and a last one for the end of the scope:
         final      destinations with no recorded stage pending          pending   the table: destination names in order
         applied    the steps (item indices) whose write has happened, in the order the writes happen
         flush      None | 'table' | 'clash' | 'direct' | 'flush' | 'exit'   slot / vec  of a stage recorded by this item
    flush_before_direct=False: the rule before this fuzz existed (a direct write leaves the table alone)."""
    table, applied, out, depth = [], [], [], 0
    names = list(seq.dests)

    def flush():
        applied.extend(i for i, _ in table)
        del table[:]

    for i, it in enumerate(seq.items):
        ev = dict(flush=None, slot=None, vec=None, recorded=False)
        if isinstance(it, Step):
            d = seq.dests[it.dest]
            recording = (not seq.outer) or depth > 0
            hit = any(overlap(d, seq.dests[n]) for _, n in table)
            if two_stage(it) and recording and it.defer:
                if len(table) == SLAB_MAXD or hit:
                    ev['flush'] = 'table' if len(table) == SLAB_MAXD else 'clash'
                    flush()
                ev.update(slot=len(table), vec=vec_stage(seq, it), recorded=True)
                table.append((i, it.dest))
            else:
                if hit and flush_before_direct:
                    ev['flush'] = 'direct'
                    flush()
                applied.append(i)
        elif it[0] == 'inner+':
            depth += 1
        elif it[0] == 'inner-':
            depth -= 1
            assert depth >= 0
        elif it[0] == 'flush':
            ev['flush'] = 'flush'
            flush()
        else:
            assert it[0] == 'check', it
        pend = tuple(n for _, n in table)
        out.append(dict(ev, final=frozenset(n for n in names if n not in pend), pending=pend, applied=tuple(applied)))
    assert depth == 0
    flush()
    out.append(dict(flush='exit', slot=None, vec=None, recorded=False, final=frozenset(names), pending=(),
                    applied=tuple(applied)))
    return out


def model(seq):
    """after every item (and, last, after the scope): the set of destinations that are final"""
    return [t['final'] for t in trace(seq)]


def seen_of(seqs):
    """the coverage classes a list of sequences reaches: what they declare and what their traces show"""
    seen = set()
    for q in seqs:
        seen |= q.tags
        tr = trace(q)
        scalars = 0                                  # scalar descriptors in front of this one in its table
        for (i, it), t in zip(enumerate(q.items), tr):
            if t['flush']:
                seen.add(('flush', t['flush']))
            if t['recorded']:
                seen.add(('slot', t['slot'], 'vec' if t['vec'] else 'scalar'))
                d = q.dests[it.dest]
                scalars = 0 if t['slot'] == 0 else scalars
                if t['vec'] and d.ld != d.ncol and scalars:
                    seen.add('pitched vector stage behind scalar ones')
                scalars += 0 if t['vec'] else 1
            if isinstance(it, Step):
                seen.add(('stage', label(it, q.dests[it.dest]), 'recorded' if t['recorded'] else 'at once'))
    return seen


def required():
    need = set(['z sweep', 'table', 'clash', 'mixed', 'scope', 'gemm_h', 'pitched vector stage behind scalar ones'])
    need |= set(('z', Z, v, acc, pos) for Z in Z_SWEEP for v in ('vec', 'scalar') for acc in (0, 1)
                for pos in ('alone', 'last of five'))
    need |= set(('table', n) for n in TABLE_SIZES)
    need |= set(('slot', k, v) for k in range(SLAB_MAXD) for v in ('vec', 'scalar'))
    need |= set(('clash', 'same output', a, b) for a, b in ACC_PAIRS)
    need |= set([('clash', 'column blocks'), ('clash', 'adjacent'), ('clash', 'inside span')])
    for order in ('two-stage then direct', 'direct then two-stage'):
        for defer2 in (True, False):
            need |= set([('mixed', 'col_sum', (1, 1), order, defer2), ('mixed', 'col_sum', (1, 0), order, defer2),
                         ('mixed', 'gemm', (1, 1), order, defer2), ('mixed', 'gemm_h', (1, 1), order, defer2)])
        need.add(('mixed', 'channel_sum', (1, 1), order, True))
    need |= set(('scope', s) for s in ('owner', 'outer', 'flush', 'side stream'))
    need |= set(('gemm_h', f) for f in ('c', 'pv', 'ps'))
    need |= set(('flush', r) for r in ('table', 'clash', 'direct', 'flush'))
    for kind in ('col_sum', 'channel_sum', 'gemm', 'gemm_h'):
        pit = (' contiguous', ' pitched') if kind in ('gemm', 'gemm_h') else ('',)
        for p in pit:
            need.add(('stage', '%s two-stage%s' % (kind, p), 'recorded'))
        need.add(('stage', '%s direct%s' % (kind, pit[-1]), 'at once'))
        if kind != 'channel_sum':
            need.add(('stage', '%s two-stage%s' % (kind, pit[-1]), 'at once'))   # defer=False: the pause path
    need.add(('stage', 'conv_wgrad two-stage', 'recorded'))
    return need


def coverage(seen):
    missing = sorted(repr(c) for c in required() - set(seen))
    assert not missing, 'the sequence lists no longer reach: %s' % ', '.join(missing)


# ---------------------------------------------------------------------------------------------------------------------
# values
# ---------------------------------------------------------------------------------------------------------------------
def _draw(pas, gen):
    if pas is EXACT:
        return lambda *shape: torch.randint(1, 4, shape, generator=gen).float()
    return lambda *shape: torch.randn(*shape, generator=gen)


def make_inputs(seq, pas, seed=7):
    """(inputs per step index, start per destination): CPU fp32; the operands of gemm_h hold bf16 values"""
    gen = torch.Generator().manual_seed(seed)
    d = _draw(pas, gen)
    inputs = {}
    for i, s in seq.steps():
        p = s.p
        sc = 1.0 if pas is EXACT else red_len(s) ** -0.5
        if s.kind == 'col_sum':
            t = [d(p['M'], p['N']) * sc]
        elif s.kind == 'channel_sum':
            t = [d(p['B'], p['C'], p['L']) * sc]
        elif s.kind == 'conv_wgrad':
            t = [d(p['B'], p['A'], p['Lsh']) * sc, d(p['B'], p['C'], p['Lsh'])]
        else:
            t = [d(p['K'], p['M']) * sc, d(p['K'], p['N'])]
            if s.kind == 'gemm_h':
                t = [x.bfloat16().float() for x in t]
        inputs[i] = t
    starts = {}
    for n, dd in seq.dests.items():
        if seq.first_acc(n):
            v = d(dd.rows, dd.ncol)
            if pas is EXACT:
                v = v * (1 - 2 * torch.randint(0, 2, v.shape, generator=gen).float())
            else:
                v = v + torch.where(v >= 0, torch.ones_like(v), -torch.ones_like(v)) * 0.5
            assert bool((v != 0).all())
        else:
            v = torch.full((dd.rows, dd.ncol), float('nan'))
        starts[n] = v
    return inputs, starts


def value(s, inp, dtype):
    """what one call adds to (or puts into) its destination, from its contract, in `dtype`"""
    p = s.p
    x = [t.to(dtype) for t in inp]
    if s.kind == 'col_sum':                      # out[n] (+)= sum_m X[m, n]
        return x[0].sum(0).view(1, -1)
    if s.kind == 'channel_sum':                  # db[c] (+)= sum_{b,t} dy[b,c,t]
        return x[0].sum((0, 2)).view(1, -1)
    if s.kind == 'conv_wgrad':                   # dw[a,c,k] += sum_{b,t} sh[b,a,t] lg[b,c,t+k-1]   (K 3, stride 1, pad 1)
        lp = F.pad(x[1], (1, 1))
        L = p['Lsh']
        return torch.stack([torch.einsum('bat,bct->ac', x[0], lp[:, :, k:k + L]) for k in range(3)], 2).reshape(1, -1)
    return x[0].t() @ x[1]                       # C = A^T B + beta C


def reference(seq, inputs, starts, dtype=torch.float64, applied=None):
    """every destination after the steps `applied` (item indices, in this order; default: all, in sequence order)"""
    img = dict((n, v.to(dtype).clone()) for n, v in starts.items())
    order = [i for i, _ in seq.steps()] if applied is None else applied
    for i in order:
        s = seq.items[i]
        v = value(s, inputs[i], dtype)
        img[s.dest] = img[s.dest] + v if s.acc else v
    return img


# ---------------------------------------------------------------------------------------------------------------------
# running a sequence
# ---------------------------------------------------------------------------------------------------------------------
def _bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


class Placed(object):
    """the frames of one run: destinations at their starts, what is left of each frame at REST"""

    def __init__(self, seq, starts, device):
        self.seq, self.fr = seq, {}
        for name, g in seq.frames.items():
            if g[0] == 'flat':
                fill = torch.full((g[1],), REST)
                f = CC.FlatFrame((g[1],), device, fill)
            else:
                _, rows, width, ld, off = g
                assert ld >= width
                fill = torch.full((rows, width), REST)
                f = CC.StridedFrame((rows, width), (ld, 1), off, device, fill)
            self.fr[name] = f
        for n in seq.dests:
            self.view(n).copy_(starts[n])
        for f in self.fr.values():               # (the frames' own guard check compares with `before`: leave it as built)
            assert f.untouched()

    def view(self, n):
        d = self.seq.dests[n]
        w = self.fr[d.frame].win
        if w.dim() == 1:
            assert d.ld == d.ncol
            return w[d.off:d.off + d.rows * d.ncol].view(d.rows, d.ncol)
        r0, c0 = divmod(d.off, w.stride(0))
        assert c0 + d.ncol <= w.size(1) and r0 + d.rows <= w.size(0) and (d.rows == 1 or d.ld == w.stride(0))
        return w[r0:r0 + d.rows, c0:c0 + d.ncol]

    def snapshot(self):
        return dict((n, self.view(n).detach().cpu().clone()) for n in self.seq.dests)

    def rest_ok(self):
        """guards untouched, and every float of a frame that is no destination's still REST"""
        for name, f in self.fr.items():
            if not f.untouched():
                return False
            w = f.window()
            mask = torch.ones(w.shape, dtype=torch.bool)
            for n, d in self.seq.dests.items():
                if d.frame != name:
                    continue
                if w.dim() == 1:
                    mask[d.off:d.off + d.rows * d.ncol] = False
                else:
                    r0, c0 = divmod(d.off, self.fr[name].win.stride(0))
                    mask[r0:r0 + d.rows, c0:c0 + d.ncol] = False
            if not bool((w[mask] == REST).all()):
                return False
        return True


def place_inputs(seq, inputs, device):
    """every operand in a frame filled with 99; returns (tensors per step, the frames)"""
    placed, frames = {}, []
    for i, s in seq.steps():
        row = []
        for t in inputs[i]:
            if s.kind == 'gemm_h':
                f = CC.FlatFrame(tuple(t.shape), device, t.bfloat16(), dtype=torch.bfloat16)
            else:
                st = [1] * t.dim()
                for k in range(t.dim() - 2, -1, -1):
                    st[k] = st[k + 1] * t.size(k + 1)
                f = CC.StridedFrame(tuple(t.shape), tuple(st), 0, device, t, sentinel=99.0)
            frames.append(f)
            row.append(f.win)
        placed[i] = row
    return placed, frames


def call(Kmod, s, dst, x):
    p = s.p
    if s.kind == 'col_sum':
        out = dst.reshape(-1)
        assert out.data_ptr() == dst.data_ptr()
        Kmod.col_sum(x[0], out, accumulate=bool(s.acc), defer=s.defer)
    elif s.kind == 'channel_sum':
        out = dst.reshape(-1)
        assert out.data_ptr() == dst.data_ptr()
        Kmod.channel_sum(x[0], out, accumulate=bool(s.acc))
    elif s.kind == 'conv_wgrad':
        out = dst.reshape(-1).view(p['A'], p['C'], 3)
        assert out.data_ptr() == dst.data_ptr()
        Kmod.conv_wgrad(x[0], x[1], out, 3, 1, 1)
    elif s.kind == 'gemm':
        Kmod.gemm(x[0], x[1], dst, ta=True, beta=float(s.acc), defer=s.defer)
    else:
        assert s.kind == 'gemm_h'
        Kmod.gemm_h(x[0], x[1], C=dst, ta=True, beta=float(s.acc), defer=s.defer)


def run(Kmod, seq, inputs, starts, device, scoped):
    """returns dict(final= every destination, snaps= {checkpoint: every destination} (scoped runs), intact= bool)"""
    gpu = str(device) != 'cpu'
    pl = Placed(seq, starts, device)
    x, xfr = place_inputs(seq, inputs, device)
    snaps = {}

    def body():
        blocks = []
        for i, it in enumerate(seq.items):
            if isinstance(it, Step):
                call(Kmod, it, pl.view(it.dest), x[i])
            elif not scoped:
                continue
            elif it[0] == 'inner+':
                blocks.append(Kmod.deferred_reduces())
                blocks[-1].__enter__()
            elif it[0] == 'inner-':
                blocks.pop().__exit__(None, None, None)
            elif it[0] == 'flush':
                Kmod.flush_reduces()
            elif it[0] == 'check':
                if gpu:
                    torch.cuda.synchronize()
                snaps[it[1]] = pl.snapshot()

    def scope():
        if scoped:
            with Kmod.deferred_reduces(outer=seq.outer):
                body()
        else:
            body()

    if gpu and seq.stream:
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            scope()
        side.synchronize()
    else:
        scope()
        if gpu:
            torch.cuda.synchronize()
    return dict(final=pl.snapshot(), snaps=snaps, intact=pl.rest_ok() and all(f.untouched() for f in xfr))


def rel_err(got, ref):
    return float((got.double() - ref).abs().max()) / max(float(ref.abs().max()), 1e-30)


def check_seq(Kmod, seq, device, worst=None, seed=7, pending=True):
    """the assertions of the fuzz for one sequence, both passes.  `pending`: the library under test really defers (the CPU
    model does not), so the checkpoints are compared with the model of the recording rules."""
    tr = trace(seq)
    for pas in (EXACT, REAL):
        tag = '%s [%s]' % (seq.name, pas['name'])
        inputs, starts = make_inputs(seq, pas, seed)
        ref = reference(seq, inputs, starts)
        plain = run(Kmod, seq, inputs, starts, device, False)
        first = run(Kmod, seq, inputs, starts, device, True)
        again = run(Kmod, seq, inputs, starts, device, True)
        for r, what in ((plain, 'plain'), (first, 'scoped'), (again, 'scoped again')):
            assert r['intact'], '%s: %s run wrote outside its destinations' % (tag, what)
        for n in seq.dests:
            assert not bool(torch.isnan(plain['final'][n]).any()), '%s: %s holds a NaN after the plain run' % (tag, n)
            assert same_bits(first['final'][n], plain['final'][n]), \
                '%s: %s differs between the scoped and the plain run\n%s\n%s' % (tag, n, first['final'][n], plain['final'][n])
            assert same_bits(again['final'][n], first['final'][n]), '%s: %s differs between two scoped runs' % (tag, n)
        if pending:
            for i, it in enumerate(seq.items):
                if isinstance(it, Step) or it[0] != 'check':
                    continue
                t, snap = tr[i], first['snaps'][it[1]]
                now = reference(seq, inputs, starts, applied=list(t['applied']))
                for n in seq.dests:
                    touched = any(seq.items[j].dest == n for j in t['applied'])
                    state = 'final' if n in t['final'] else 'pending'
                    if not touched:
                        assert same_bits(snap[n], starts[n]), \
                            '%s, checkpoint %s: %s (%s) must still hold its start\n%s' % (tag, it[1], n, state, snap[n])
                    elif pas is EXACT:
                        assert torch.equal(snap[n].double(), now[n]), \
                            '%s, checkpoint %s: %s (%s) is not what the steps that are final give\n%s\n%s' % (
                                tag, it[1], n, state, snap[n], now[n])
                    elif n in t['final'] and not any(seq.items[j].dest == n for j, _ in seq.steps() if j > i):
                        assert same_bits(snap[n], first['final'][n]), '%s, checkpoint %s: %s is final but changed later' % (
                            tag, it[1], n)
        if pas is EXACT:
            for n in seq.dests:
                assert torch.equal(plain['final'][n].double(), ref[n]), \
                    '%s: %s is not the float64 reference\n%s\n%s' % (tag, n, plain['final'][n], ref[n])
            continue
        low = reference(seq, inputs, starts, dtype=torch.float32)
        for n, d in seq.dests.items():
            floor = max(rel_err(low[n], ref[n]), CC.FLOOR_MIN)
            err = rel_err(plain['final'][n], ref[n])
            labels = sorted(set(label(s, d) for _, s in seq.steps() if s.dest == n))
            margin = max(MARGINS.get(lb, (MARGIN,))[0] for lb in labels)
            assert MARGIN <= margin <= CC.MARGIN_MAX
            print('  %-52s %-24s %-36s err %.3g floor %.3g ratio %.2f' % (seq.name, n, ' + '.join(labels), err, floor, err / floor))
            if worst is not None:
                for lb in labels:
                    worst[lb] = max(worst.get(lb, 0.0), err / floor)
            assert err <= CC.bound(margin, floor), '%s: %s error %.3g above %g x floor %.3g' % (tag, n, err, margin, floor)
