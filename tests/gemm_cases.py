"""Shared pieces of the GEMM dispatch fuzz (test_gemm_fuzz.py on the GPU, test_gemm_fuzz_host.py against the CPU model)
--  TEST INFRASTRUCTURE, no test functions.

  cases() / cases_h()   a pinned list (one case per dispatch form the coverage assertions name) followed by seeded random
                        cases: (M, N, K, ta, tb, opts).  The size pools straddle every threshold of ag_gemm, ag_gemm_h
                        and gemm_pick_ksplit (32 / 64 / 128 rows, K 1024 / 2048, K % 4, K % 16, K % 64, rows % 4, % 8);
                        they are the smallest shapes that reach each branch, none is a workload size.
  make_inputs()         the operands of one case for one PASS:
                          EXACT  integers in [-3, 3], alpha in {1, 0.5, -2}, beta in {0, 1, -0.5}, slope 0.5, no tanh.  With
                                 K <= 8192 every partial sum is an integer below 2^17, so every fp32 summation order is exact,
                                 bf16 holds the operands exactly and the f32x3 low parts are zero: the result must equal the
                                 float64 reference BIT FOR BIT (a bf16 output: its round-to-nearest-even image).  Zero
                                 tolerance catches a dropped, doubled or misplaced k element or output element anywhere.
                          REAL   randn operands (A scaled by K^-1/2 so that the product is of the size of the epilogue's
                                 addends and an epilogue error is as visible as a product error), alpha / beta / slope that
                                 are no powers of two, tanh included.  Under tanh every addend is scaled by another 1/4: the
                                 bounds are fractions of the OUTPUT scale, tanh caps that at 1 while the absolute error of the
                                 pre-activation passes through unchanged where tanh is steep, so the pre-activation has to
                                 stay of order 1 for the declared bounds to mean what they mean for a linear epilogue.
  reference()           float64, from the contract in include/audiogan_hip.h, on the operand values the mode defines.
  run()                 places operands / output as the case says (column blocks of wider tensors, aligned or not, a base
                        shifted by one element), the output inside a sentinel-filled frame (two rows above and below, the
                        pitch padding left and right), the window pre-filled with NaN when beta == 0; calls the kernel;
                        returns the window(s) and whether the frame is bit-for-bit untouched.
  check()               the assertions of one pass; bounds are the project's declared ones.
  gemm_plan() / gemm_h_plan()   a restatement of the dispatch conditions of gemm.hip / gemm_bf16s.hip on sizes alone.  The
                        GPU tests assert coverage on the kernel names the LIBRARY reports (ag_last_kernel) and on
                        ag_gemm_ws_numel; the plan is what the host test uses to show that the seeded list holds the shape
                        classes those assertions need, and what a mutant of the host test slices K by.
"""
import torch

ACT_NONE, ACT_LEAKY, ACT_TANH, ACT_LEAKY_GATE = 0, 1, 2, 3

M_POOL = (1, 5, 33, 64, 65, 100, 128, 129, 200, 256, 260, 384, 520)
K_POOL = (1, 5, 16, 24, 29, 36, 64, 200, 1000, 1024, 1040, 1480, 2048, 2050, 4096, 8192)
K_POOL_H = (64, 128, 192, 1024, 1088, 2048, 4096, 8192)
MNK_MAX = 1.2e9          # per case; a test function's list sums to about 2e10 (host test: asserted)

EXACT = dict(name='exact', alpha=(1.0, 0.5, -2.0), beta=(0.0, 1.0, -0.5), slope=0.5)
REAL = dict(name='real', alpha=(1.0, 0.7, -1.3), beta=(0.0, 1.0, -0.45), slope=0.3)

PAD_ROWS = 2
SENTINEL = -12345.0       # (a bf16 frame holds its rounded value: a frame is compared with its own image from before the call)


def cdiv(a, b):
    return (a + b - 1) // b


def roundup(a, b):
    return cdiv(a, b) * b


def opts(alpha=0, beta=0, bias=0, res=0, act=ACT_NONE, view=0, misalign=0, out='c', res16=0, gate=0):
    """alpha / beta: index into the pass's value table;  bias: 0 none, 1 its own tensor, 2 a view offset by one float;
    view: 0 contiguous, 1 column blocks at offset 8 with a pitch % 4 == 0, 2 at offset 3 with an odd pitch (ag_gemm_h:
    operands stay in the aligned form, which ag_gemm_h requires; the output / residual / gate take the unaligned one);
    misalign: operand bases shifted by one element (ag_gemm only);  out / res16 / gate: ag_gemm_h only"""
    if act == ACT_LEAKY_GATE:
        res = 1                    # the gate's saved activation travels in `res`
    return dict(alpha=alpha, beta=beta, bias=bias, res=res, act=act, view=view, misalign=misalign, out=out, res16=res16,
                gate=gate)


# ---------------------------------------------------------------------------------------------------------------------
# the dispatch, restated on sizes (gemm.hip: ag_gemm, gemm_pick_ksplit, gemm_pick_tile; gemm_bf16s.hip: ag_gemm_h)
# ---------------------------------------------------------------------------------------------------------------------
def pick_ksplit(tiles, mn, K):
    want = (512 * 4 // tiles + 2) // 3
    for c in (32, 24, 16, 8, 4, 2):
        if c <= want and c <= K // 256 and c * mn <= (12 << 20):
            return c
    return 1


TILE_SHAPES = ((128, 128, 2, 2), (256, 128, 2, 2), (128, 256, 2, 2), (256, 256, 2, 4))


def pick_tile(M, N, ksplit):
    rate = (120., 133., 133., 137.)
    best, best_t = 0, 0.
    for s in (3, 1, 2, 0):
        bm, bn = TILE_SHAPES[s][:2]
        wgs = cdiv(M, bm) * cdiv(N, bn) * ksplit
        t = float(cdiv(wgs, 256)) * bm * bn / rate[s] + 1e-9 * float(wgs) * bm * bn
        if best_t == 0. or t < best_t * 0.98:
            best, best_t = s, t
    return best


def split_eligible(M, N, K, act):
    """ag_gemm_ws_numel(M, N, K, act) > 0"""
    return gemm_ws_numel(M, N, K, act) > 0


def gemm_ws_numel(M, N, K, act):
    big = cdiv(M, 128) * cdiv(N, 128)
    use128 = M > 64 and N > 64 and (big >= 192 or K >= 2048)
    tiles = big if use128 else cdiv(M, 64) * cdiv(N, 64)
    if not (tiles < 192 and K >= 1024 and act == ACT_NONE):
        return 0
    ks = pick_ksplit(tiles, M * N, K)
    return ks * M * N if ks >= 2 else 0


def _block(cols, view, q=4):
    """(column offset, row pitch) of a [rows, cols] column block in the form `view`; q: elements per 16 bytes"""
    if view == 0:
        return 0, cols
    if view == 1:
        return 2 * q, roundup(cols + 3 * q, q)
    return 3, (cols + 7) | 1


def operand_vec(cols, o):
    """does ag_gemm read an operand stored [rows][cols] in 16-byte pieces?  (16-byte aligned base, pitch % 4 == 0)"""
    off, ld = _block(cols, o['view'])
    return (not o['misalign']) and off % 4 == 0 and ld % 4 == 0


def gemm_plan(mode, M, N, K, ta, tb, o, act=None, ws_numel=None):
    """kernel name, K slices and tile of ag_gemm for this case in precision `mode` ('f32' / 'bf16' / 'f32x3')"""
    act = o['act'] if act is None else act
    vec = operand_vec(M if ta else K, o) and operand_vec(K if tb else N, o)
    big = cdiv(M, 128) * cdiv(N, 128)
    use128 = M > 64 and N > 64 and (big >= 192 or K >= 2048)
    tiles = big if use128 else cdiv(M, 64) * cdiv(N, 64)
    ksplit, kchunk, mn = 1, roundup(K, 64), M * N
    if tiles < 192 and K >= 1024 and act == ACT_NONE:
        ks = pick_ksplit(tiles, mn, K)
        if ws_numel is None:
            ws_numel = ks * mn if ks >= 2 else 0
        slabs = ws_numel > 0 and ws_numel >= 2 * mn
        if slabs and ks * mn > ws_numel:
            ks = ws_numel // mn
        if ks >= 2 and slabs:
            kchunk = roundup(cdiv(K, ks), 64)
            ksplit = cdiv(K, kchunk)
    rb, x3 = mode == 'bf16', mode == 'f32x3' and use128
    rows4 = (not ta or M % 4 == 0) and (tb or N % 4 == 0)
    if (rb or x3) and M > 32 and N > 32 and vec and K % 4 == 0 and rows4:
        name, bm, bn = 'gemm_bf16_kernel<%d,%d,%d>' % (ta, tb, int(x3)), 128, 128
    elif use128 and vec and K % 16 == 0 and rows4 and not rb:
        bm, bn, ti, tj = TILE_SHAPES[pick_tile(M, N, ksplit)]
        name = 'gemm_tile_kernel<%d,%d,%d,%d,%d,%d>' % (ta, tb, bm, bn, ti, tj)
    elif use128:
        name, bm, bn = 'gemm_kernel<2,2,2,2,%d,%d>' % (ta, tb), 128, 128
    else:
        name, bm, bn = 'gemm_kernel<1,1,2,2,%d,%d>' % (ta, tb), 64, 64
    return dict(kernel=name, ksplit=ksplit, kchunk=kchunk, bm=bm, bn=bn, scalar=not vec)


def gemm_h_ok(M, N, K, ta, tb):
    return K >= 64 and K % 64 == 0 and (not ta or (M % 8 == 0 and M >= 8)) and (tb or (N % 8 == 0 and N >= 8))


def gemm_h_ws_numel(M, N, K, act, has_c16):
    tiles = cdiv(M, 128) * cdiv(N, 128)
    if not (tiles < 192 and K >= 1024 and act == ACT_NONE and not has_c16):
        return 0
    ks = pick_ksplit(tiles, M * N, K)
    return ks * M * N if ks >= 2 else 0


def gemm_h_plan(M, N, K, ta, tb, o):
    """K slices of ag_gemm_h as kernels.gemm_h drives it, and whether its full tiles take the `fast` (LDS-transposed,
    16-byte stores) epilogue"""
    has_c16 = o['out'] != 'c'
    nws = 0 if o['gate'] else gemm_h_ws_numel(M, N, K, o['act'], has_c16)
    ksplit, kchunk = 1, K
    if nws > 0 and not o['res16']:          # (a bf16 residual has no second stage: the product runs unsplit)
        kchunk = roundup(cdiv(K, nws // (M * N)), 64)
        ksplit = cdiv(K, kchunk)
    aligned = o['view'] != 2 and _block(N, o['view'])[1] % 4 == 0 and o['bias'] != 2
    return dict(kernel='gemm_bf16s_kernel<%d,%d>' % (ta, tb), ksplit=ksplit, kchunk=kchunk, bm=128, bn=128,
                fast=ksplit == 1 and aligned, eligible=nws > 0)


def tile_of(name):
    """(BM, BN) of a kernel name as ag_last_kernel reports it"""
    base, args = name.rstrip('>').split('<')
    a = [int(x) for x in args.split(',')]
    if base == 'gemm_kernel':
        return 32 * a[0] * a[2], 32 * a[1] * a[3]
    if base == 'gemm_tile_kernel':
        return a[2], a[3]
    assert base in ('gemm_bf16_kernel', 'gemm_bf16s_kernel'), name
    return 128, 128


def has_interior(M, N, bm, bn):
    return M >= bm and N >= bn


def has_ragged(M, N, bm, bn):
    return M % bm != 0 or N % bn != 0


# ---------------------------------------------------------------------------------------------------------------------
# the case lists
# ---------------------------------------------------------------------------------------------------------------------
N_, L_, T_, G_ = ACT_NONE, ACT_LEAKY, ACT_TANH, ACT_LEAKY_GATE

# ag_gemm: one case per form the coverage assertions of test_gemm_random_cases name (fp32 mode / bf16 mode / f32x3 mode)
PINNED = [
    # LDS-DMA 128 x 128 / gemm_bf16_kernel<.,.,0> / <.,.,1>: each layout, each activation on interior tiles
    (128, 256, 2048, 0, 1, opts(alpha=1, beta=2, bias=1, res=1, act=L_)),
    (260, 256, 2048, 1, 0, opts(alpha=2, beta=1, bias=2, res=1, act=T_, view=1)),
    (128, 128, 4096, 1, 1, opts(beta=0, bias=1, act=G_)),
    (256, 132, 2048, 0, 0, opts(alpha=1, res=1, act=N_)),                              # split-K, interior + ragged slabs
    # split-K in every layout: ragged tiles, K no multiple of the slice, a full second stage, a pitched C
    (200, 132, 4096, 0, 1, opts(alpha=2, beta=2, bias=1, res=1, view=1)),
    (200, 132, 1480, 1, 0, opts(alpha=1, beta=1, view=1)),                             # 64-tile kernel, slices of 384 of 1480
    (132, 200, 2048, 1, 1, opts(beta=2, bias=2, res=1)),
    (65, 260, 8192, 0, 0, opts(alpha=1, res=1, view=2)),                               # scalar loads, unaligned pitched C
    (64, 33, 1024, 1, 0, opts(beta=1, bias=1)),                                        # one 64-tile, 4 slices of 256
    # 128-tile register-staged kernel: K % 16 != 0 (bf16 mode: K % 4 != 0, operands rounded in registers), rows % 4 != 0,
    # scalar loaders (odd pitch; base shifted by one element)
    (129, 200, 2050, 0, 1, opts(alpha=2, beta=2, bias=1, res=1, act=L_)),
    (130, 129, 2050, 1, 0, opts(alpha=1, bias=1, act=T_)),
    (200, 260, 2048, 0, 0, opts(beta=2, res=1, act=G_, misalign=1)),
    (256, 128, 2048, 1, 1, opts(alpha=1, beta=1, bias=1, act=L_, view=2)),
    (129, 129, 2050, 1, 1, opts(res=1)),                                               # split-K on the 128-tile kernel
    (128, 128, 2050, 0, 0, opts(alpha=2, act=L_, view=1)),                             # interior only
    # 64-tile kernel: interior only / ragged only / scalar loads
    (64, 128, 64, 0, 1, opts(alpha=1, beta=2, bias=1, res=1, act=T_)),
    (33, 5, 29, 0, 0, opts(beta=1, res=1, act=N_)),
    (100, 65, 200, 1, 1, opts(alpha=2, bias=1, act=L_, misalign=1)),
    (65, 100, 36, 1, 0, opts(beta=2, act=G_, view=2)),
]

# ag_gemm_h
PINNED_H = [
    # full tiles through the `fast` epilogue and through the element-wise one (unaligned view, ldc % 4 != 0, bias + 1)
    (128, 256, 128, 0, 1, opts(alpha=1, beta=2, bias=1, res=1, act=L_, out='both', view=1)),
    (256, 128, 64, 1, 0, opts(bias=1, res=1, res16=1, act=T_, out='c16', gate=1)),
    (128, 128, 192, 0, 0, opts(alpha=2, beta=1, bias=1, res=1, act=N_, out='c', view=2)),
    (136, 130, 64, 1, 1, opts(res=1, res16=1, act=G_, out='c16')),                       # ldc = 130
    (256, 256, 128, 0, 1, opts(alpha=1, bias=2, act=L_, out='both')),
    # split-K with ragged tiles in every layout, with and without a second-stage epilogue
    (200, 136, 2048, 0, 1, opts(alpha=2, beta=2, bias=1, res=1, view=1)),
    (200, 136, 1088, 1, 0, opts()),                                                      # 4 slices of 320 of 1088
    (136, 200, 4096, 1, 1, opts(alpha=1, beta=1)),
    (65, 264, 1024, 0, 0, opts(beta=2, bias=2, res=1, view=2)),
    # split-eligible with a bf16 residual: must compute (unsplit), not raise
    (1024, 512, 1024, 0, 1, opts(res=1, res16=1)),
    (5, 33, 64, 0, 1, opts(alpha=2, bias=1, act=G_, out='both', res16=1, gate=1)),
]


# test_gemm_large_tiles: the three wider tiles of gemm_tile.h are chosen by gemm_pick_tile for large outputs only (more than
# 256 / 768 tiles of 128 x 128).  One shape per tile, ragged in both directions, rows % 4 == 0 so that every layout stays on
# the LDS-DMA kernel:  ((M, N, K), (BM, BN, TI, TJ))
LARGE_TILES = (((2080, 2092, 48), (256, 128, 2, 2)), ((260, 20404, 16), (128, 256, 2, 2)), ((3600, 3700, 48), (256, 256, 2, 4)))


def _draw(n, seed, h):
    gen = torch.Generator().manual_seed(seed)

    def ri(lo, hi):
        return int(torch.randint(lo, hi + 1, (1,), generator=gen))

    def pick(pool):
        return pool[ri(0, len(pool) - 1)]
    out = list(PINNED_H if h else PINNED)
    while len(out) < n:
        pool = K_POOL_H if h else K_POOL
        if ri(0, 1):                        # every other case has a long reduction: the 128-tile kernels and split-K
            pool = [k for k in pool if k >= 1024]
        M, N, K = pick(M_POOL), pick(M_POOL), pick(pool)
        ta, tb = ri(0, 1), ri(0, 1)
        o = opts(alpha=ri(0, 2), beta=ri(0, 2), bias=ri(0, 2), res=ri(0, 1), act=ri(0, 3), view=ri(0, 2),
                 misalign=0 if h else int(ri(0, 3) == 0), out=('c', 'c16', 'both')[ri(0, 2)] if h else 'c',
                 res16=ri(0, 1) if h else 0, gate=int(ri(0, 3) == 0) if h else 0)
        if h and o['out'] == 'c16':
            o['beta'] = 0                   # beta needs the fp32 output
        if h and not o['res']:
            o['res16'] = 0
        if M * N * K > MNK_MAX or (h and not gemm_h_ok(M, N, K, ta, tb)):
            continue
        out.append((M, N, K, ta, tb, o))
    return out


def cases(n=60, seed=41):
    return _draw(n, seed, False)


def cases_h(n=60, seed=43):
    return _draw(n, seed, True)


# ---------------------------------------------------------------------------------------------------------------------
# inputs, reference, runner, checker
# ---------------------------------------------------------------------------------------------------------------------
def pass_act(o, pas):
    """the exact pass has no tanh: a tanh case runs LeakyReLU there (as non-linear, so the same dispatch)"""
    return ACT_LEAKY if (pas is EXACT and o['act'] == ACT_TANH) else o['act']


def make_inputs(case, pas, seed, h=False):
    """CPU tensors of one case: A, B in their stored layout, C0, bias, res, gate (None where the case has none)"""
    M, N, K, ta, tb, o = case
    gen = torch.Generator().manual_seed(seed)
    sa, sb = ((K, M) if ta else (M, K)), ((N, K) if tb else (K, N))
    if pas is EXACT:
        def draw(*s):
            return torch.randint(-3, 4, s, generator=gen).float()
        A, B = draw(*sa), draw(*sb)
    else:
        q = 0.25 if o['act'] == ACT_TANH else 1.0

        def draw(*s):
            return torch.randn(*s, generator=gen) * q
        A, B = draw(*sa) / K ** 0.5, torch.randn(*sb, generator=gen)
    inp = dict(A=A, B=B, C0=draw(M, N), bias=draw(N) if o['bias'] else None, res=draw(M, N) if o['res'] else None,
               gate=draw(M, N) if o['gate'] else None)
    if h:
        inp['A'], inp['B'] = A.bfloat16(), B.bfloat16()
        if o['res16']:
            inp['res'] = inp['res'].bfloat16()
        if o['gate']:
            inp['gate'] = inp['gate'].bfloat16()
    return inp


def reference(case, pas, inp, rounded=False):
    """float64: act(alpha * op(A) op(B) + beta * C0 + bias + res), the gate forms, gate16 after bias / res / act.
    rounded: the operands of the product as bf16 mode defines them (rounded to nearest even)"""
    M, N, K, ta, tb, o = case
    A, B = inp['A'], inp['B']
    if rounded:
        A, B = A.bfloat16(), B.bfloat16()
    A, B = A.double(), B.double()
    v = pas['alpha'][o['alpha']] * ((A.t() if ta else A) @ (B.t() if tb else B))
    beta, slope, act = pas['beta'][o['beta']], pas['slope'], pass_act(o, pas)
    if beta != 0.0:
        v = v + beta * inp['C0'].double()
    if inp['bias'] is not None:
        v = v + inp['bias'].double().view(1, -1)
    if act == ACT_LEAKY_GATE:
        v = torch.where(inp['res'].double() > 0, v, v * slope)
    else:
        if inp['res'] is not None:
            v = v + inp['res'].double()
        if act == ACT_LEAKY:
            v = torch.where(v > 0, v, v * slope)
        elif act == ACT_TANH:
            v = torch.tanh(v)
    if inp['gate'] is not None:
        v = torch.where(inp['gate'].double() > 0, v, v * slope)
    return v


def _place(t, view, shift, device, q=4):
    """t as a column block (form `view`) of a wider device tensor, or of a flat buffer that starts `shift` elements late"""
    rows, cols = t.shape
    off, ld = _block(cols, view, q)
    flat = torch.full((rows * ld + shift,), 99.0, dtype=t.dtype, device=device)
    blk = flat[shift:].view(rows, ld)[:, off:off + cols]
    blk.copy_(t)
    return blk


class Frame(object):
    """an [M, N] output window inside a sentinel-filled frame: PAD_ROWS rows above and below, the pitch padding of the
    view form left and right"""

    def __init__(self, M, N, view, dtype, device, fill):
        off, ld = _block(N, view)
        self.frame = torch.full((M + 2 * PAD_ROWS, ld), SENTINEL, dtype=dtype, device=device)
        self.win = self.frame[PAD_ROWS:PAD_ROWS + M, off:off + N]
        self.win.copy_(fill)
        self.before = self.frame.cpu().clone()
        self.sl = (slice(PAD_ROWS, PAD_ROWS + M), slice(off, off + N))

    def untouched(self):
        after, before = self.frame.cpu().clone(), self.before.clone()
        after[self.sl] = 0
        before[self.sl] = 0
        bits = torch.int32 if after.dtype == torch.float32 else torch.int16
        return torch.equal(after.view(bits), before.view(bits))

    def window(self):
        return self.win.cpu().clone()


def run(fn, case, pas, inp, device, h=False, last_kernel=None, **extra):
    """one call of `fn` (kernels.gemm / kernels.gemm_h or a model of it).  Returns dict(c, c16, frame_ok, kernel)"""
    M, N, K, ta, tb, o = case
    beta = pas['beta'][o['beta']]
    nan32 = torch.full((M, N), float('nan'))
    view_ab = (1 if o['view'] else 0) if h else o['view']
    q = 8 if h else 4
    A = _place(inp['A'], view_ab, o['misalign'], device, q)
    B = _place(inp['B'], view_ab, o['misalign'], device, q)
    bias = None
    if inp['bias'] is not None:
        bias = torch.cat([torch.zeros(4), inp['bias']]).to(device)[4:] if o['bias'] == 1 else \
            torch.cat([torch.zeros(1), inp['bias']]).to(device)[1:]
    res = _place(inp['res'], o['view'], 0, device) if inp['res'] is not None else None
    kw = dict(ta=bool(ta), tb=bool(tb), alpha=pas['alpha'][o['alpha']], beta=beta, bias=bias, res=res, act=pass_act(o, pas),
              slope=pas['slope'])
    kw.update(extra)
    f32 = f16 = None
    if not h or o['out'] != 'c16':
        f32 = Frame(M, N, o['view'], torch.float32, device, nan32 if beta == 0.0 else inp['C0'])
    if h:
        if o['out'] != 'c':
            f16 = Frame(M, N, o['view'], torch.bfloat16, device, nan32.bfloat16())
        gate = _place(inp['gate'], o['view'], 0, device) if inp['gate'] is not None else None
        fn(A, B, C=f32.win if f32 else None, C16=f16.win if f16 else None, gate=gate, **kw)
    else:
        fn(A, B, f32.win, **kw)
    name = last_kernel() if last_kernel else ''
    return dict(c=f32.window() if f32 else None, c16=f16.window() if f16 else None,
                frame_ok=(f32 is None or f32.untouched()) and (f16 is None or f16.untouched()), kernel=name,
                frames=(f32, f16))


def bound_of(mode, kernel):
    """the declared bound of the fp32 output, as a fraction of the reference's largest magnitude"""
    if mode == 'f32x3' and kernel.startswith('gemm_bf16_kernel<') and kernel.endswith(',1>'):
        return 2e-5
    return 1e-4


def check(case, pas, mode, ref, got, full=None):
    """the assertions of one pass on run()'s result; returns the fp32 output's error as a fraction of the scale.
    full: bf16 mode's unrounded-operand reference (the mode must really round: K >= 36)"""
    tag = (case, pas['name'], mode, got['kernel'])
    assert got['frame_ok'], ('wrote outside its [M, N] window', tag)
    c, c16 = got['c'], got['c16']
    if pas is EXACT:
        if c is not None:
            assert torch.equal(c, ref.float()), ('exact pass: fp32 output differs from the float64 reference', tag,
                                                 float((c.double() - ref).abs().max()))
        if c16 is not None:
            assert torch.equal(c16.float(), ref.float().bfloat16().float()), ('exact pass: bf16 output is not RNE(reference)', tag)
        return 0.0
    scale = max(float(ref.abs().max()), 1e-30)
    err = 0.0
    if c is not None:
        err = float((c.double() - ref).abs().max()) / scale
        assert err <= bound_of(mode, got['kernel']), ('real pass', tag, err)
        if full is not None and case[2] >= 36:
            far = float((c.double() - full).abs().max()) / scale
            assert far > 10 * err, ('bf16 mode did not round its operands', tag, err, far)
    if c16 is not None:
        d = (c16.double() - ref.float().bfloat16().double()).abs()
        assert float(d.max()) <= 2.0 ** -7 * scale, ('real pass: bf16 output', tag, float(d.max()) / scale)
        assert float((d > 0).double().mean()) < 0.02, ('real pass: bf16 output off its rounding', tag)
    return err


# ---------------------------------------------------------------------------------------------------------------------
# coverage: what a case list must have reached.  `seen`: [(case, kernel name, split-eligible)] - on the GPU the name is
# what ag_last_kernel reported and split-eligible is ag_gemm_ws_numel(...) > 0 / ag_gemm_h_ws_numel(...) > 0; the host
# test passes gemm_plan()'s restatement.  Every form is named here, so a change of the dispatch (or of the list) that stops
# reaching one fails instead of silently shrinking the test.
# ---------------------------------------------------------------------------------------------------------------------
LAYOUTS = ((0, 0), (0, 1), (1, 0), (1, 1))


def _need_layouts(names, fmt, what):
    missing = [fmt % l for l in LAYOUTS if fmt % l not in names]
    assert not missing, (what, 'never launched', missing)


def _family(name):
    base = name.split('<')[0]
    return base + str(tile_of(name)[0]) if base == 'gemm_kernel' else base


def _second_stage_epilogue(o):
    return bool(o['bias']) and bool(o['res']) and o['beta'] == 2


def assert_gemm_coverage(mode, seen):
    names = set(k for _, k, _ in seen)
    _need_layouts(names, 'gemm_kernel<1,1,2,2,%d,%d>', mode)      # (bf16 mode: the fp32 fallbacks on rounded operands)
    _need_layouts(names, 'gemm_kernel<2,2,2,2,%d,%d>', mode)
    if mode == 'f32':
        _need_layouts(names, 'gemm_tile_kernel<%d,%d,128,128,2,2>', mode)
    if mode == 'bf16':
        _need_layouts(names, 'gemm_bf16_kernel<%d,%d,0>', mode)
    if mode == 'f32x3':
        _need_layouts(names, 'gemm_bf16_kernel<%d,%d,1>', mode)
    fams = ['gemm_kernel64', 'gemm_kernel128', 'gemm_tile_kernel' if mode == 'f32' else 'gemm_bf16_kernel']
    for fam in fams:
        tiles =[(c, tile_of(k)) for c, k, _ in seen if _family(k) == fam]
        assert any(has_interior(c[0], c[1], *t) for c, t in tiles), (mode, fam, 'no interior tile')
        assert any(has_ragged(c[0], c[1], *t) for c, t in tiles), (mode, fam, 'no ragged tile')
    split = [(c, k) for c, k, s in seen if s]
    for l in LAYOUTS:
        assert any((c[3], c[4]) == l for c, _ in split), (mode, 'no split-K case in layout', l)
    assert any(c[0] % 128 and c[1] % 128 for c, _ in split), (mode, 'split-K: no case with ragged M and N')
    assert any(c[2] % gemm_plan(mode, *c)['kchunk'] for c, _ in split), (mode, 'split-K: no ragged last slice')
    assert any(_second_stage_epilogue(c[5]) for c, _ in split), (mode, 'split-K: no bias + res + beta second stage')
    assert any(c[5]['view'] for c, _ in split), (mode, 'split-K: no pitched C')
    if mode == 'f32':
        for act in (ACT_NONE, ACT_LEAKY, ACT_TANH, ACT_LEAKY_GATE):
            assert any(k.startswith('gemm_tile_kernel<') and c[5]['act'] == act and has_interior(c[0], c[1], *tile_of(k))
                       for c, k, _ in seen), (mode, 'activation never on an interior tile of gemm_tile_kernel', act)
    for fam in ('gemm_kernel64', 'gemm_kernel128'):
        assert any(_family(k) == fam and gemm_plan(mode, *c)['scalar'] for c, k, _ in seen), (mode, fam, 'no scalar-loader case')


def assert_gemm_h_coverage(seen):
    names = set(k for _, k, _ in seen)
    _need_layouts(names, 'gemm_bf16s_kernel<%d,%d>', 'ag_gemm_h')
    plans = [(c, c[5], gemm_h_plan(*c)) for c, _, _ in seen]
    full = [(c, o, p) for c, o, p in plans if has_interior(c[0], c[1], 128, 128) and p['ksplit'] == 1]

    def need(what, it):
        assert any(it), ('ag_gemm_h', 'never reached', what)
    need('fast epilogue', (p['fast'] for c, o, p in full))
    need('element-wise epilogue on full tiles: unaligned view', (o['view'] == 2 for c, o, p in full))
    need('element-wise epilogue on full tiles: ldc % 4 != 0', (o['view'] == 0 and c[1] % 4 != 0 for c, o, p in full))
    need('element-wise epilogue on full tiles: bias view offset by one float',
         (o['bias'] == 2 and o['view'] != 2 and _block(c[1], o['view'])[1] % 4 == 0 for c, o, p in full))
    need('ragged tiles', (has_ragged(c[0], c[1], 128, 128) for c, o, p in plans))
    need('M < 128', (c[0] < 128 for c, o, p in plans))
    for out in ('c', 'c16', 'both'):
        need('output ' + out, (o['out'] == out for c, o, p in plans))
    need('fp32 residual', (o['res'] and not o['res16'] for c, o, p in plans))
    need('bf16 residual', (o['res'] and o['res16'] for c, o, p in plans))
    need('gate', (o['gate'] for c, o, p in plans))
    need('ACT_LEAKY_GATE', (o['act'] == ACT_LEAKY_GATE for c, o, p in plans))
    need('alpha != 1', (o['alpha'] != 0 for c, o, p in plans))
    need('beta not in {0, 1}', (o['beta'] == 2 for c, o, p in plans))
    for l in LAYOUTS:
        need('split-K with ragged tiles in layout %d,%d' % l,
             (p['ksplit'] > 1 and (c[3], c[4]) == l and has_ragged(c[0], c[1], 128, 128) for c, o, p in plans))
    need('split-K with a second-stage epilogue', (p['ksplit'] > 1 and (o['bias'] or o['res'] or o['beta'] == 2) for c, o, p in plans))
    need('split-K without a second-stage epilogue',
         (p['ksplit'] > 1 and not (o['bias'] or o['res'] or o['beta'] == 2) for c, o, p in plans))
    need('split-K with a ragged last slice', (p['ksplit'] > 1 and c[2] % p['kchunk'] for c, o, p in plans))
    need('split-eligible with a bf16 residual', (e and c[5]['res16'] for c, _, e in seen))
