"""The generator front at the reference's default frame size (200) and at the padded panel width (256), S = 1024, on HIP
events: per (cell, frame size, B, T) the training forward of the front (the z/c pre-activation GEMM, the frame loop, the stop
head), its backward (frame loop + the weight-gradient products + the weight-norm backward) and Generator.generate with u = 1
(no clip stops: all T frames and the conv trunk on all of them).

    python tools/front_frames.py --json OUT.json [--root CHECKOUT] [--tag NAME]     one run: measure
    python tools/front_frames.py --table A.json B.json ...                          the table of several runs

``--root``: import audiogan_amd from another checkout (a built tree of the commit to compare against) instead of this one.
Each case is warmed up, then repeated until about ``--window`` seconds of device time are covered; the figure is the
median over the repetitions, the minimum rides along.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _time(fn, window, lo=5, hi=400):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    while len(ts) < lo or (sum(ts) < window * 1e6 and len(ts) < hi):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    ts.sort()
    return ts[len(ts) // 2], ts[0], len(ts)


def measure(a):
    sys.path.insert(0, os.path.abspath(a.root) if a.root else ROOT)
    import audiogan_amd as A
    from audiogan_amd import kernels as K, ops
    dev = torch.device('cuda')
    S, ns, es = 1024, 100, 100
    rows = []
    K.lstm_persist_status(reset=True)
    for cell in a.cells.split(','):
        for fs in [int(v) for v in a.fs.split(',')]:
            torch.manual_seed(0)
            cfg = dict(frame_size=fs, embed_size=es, noise_size=ns, state_size=S)
            g = (A.GRUGenerator(**cfg) if cell == 'gru' else A.Generator(num_layers=1, **cfg)).to(dev)
            for B in [int(v) for v in a.B.split(',')]:
                persistent = bool(g.front_is_persistent(B, dev) and K.gfront_bwd_persist_ok(B, S, fs, dev))
                for T in [int(v) for v in a.T.split(',')]:
                    z, c = torch.randn(B, T, ns, device=dev), torch.randn(B, es, device=dev)
                    zc = ops.BuildZCFn.apply(z, c)
                    gx, gs = torch.randn(B, T * fs, device=dev), torch.randn(B, T, device=dev)
                    u = torch.ones(T, B, device=dev)
                    g.refresh_weights()
                    out = {}

                    def fwd():
                        out['xs'] = g._front_apply(zc)

                    def bwd():
                        torch.autograd.backward(list(out['xs']), [gx, gs], retain_graph=True)

                    f_med, f_min, f_n = _time(fwd, a.window)
                    b_med, b_min, b_n = _time(bwd, a.window)
                    out.clear()
                    for q in g.parameters():
                        q.grad = None
                    with torch.no_grad():
                        s_med, s_min, s_n = _time(lambda: g.generate(c, z=z, u=u), a.window)
                        t_run = g.last_t_run
                    rows.append(dict(tag=a.tag, cell=cell, fs=fs, B=B, T=T, persistent=persistent,
                                     t_run=None if t_run is None else int(t_run),
                                     fwd_us=f_med, fwd_us_min=f_min, fwd_n=f_n, bwd_us=b_med, bwd_us_min=b_min, bwd_n=b_n,
                                     gen_us=s_med, gen_us_min=s_min, gen_n=s_n))
                    print('%-8s %-4s fs %3d B %2d T %3d %s  fwd %9.1f  bwd %9.1f  generate %9.1f us' % (
                        a.tag, cell, fs, B, T, 'persistent' if persistent else 'per-frame ', f_med, b_med, s_med), flush=True)
    torch.cuda.synchronize()
    assert K.lstm_persist_status() == 0, 'a persistent launch gave up'
    with open(a.json, 'w') as f:
        json.dump(rows, f, indent=1)


def table(paths):
    runs = []
    for p in paths:
        with open(p) as f:
            runs.append(json.load(f))
    names = ['%s#%d' % (r[0]['tag'], i + 1) for i, r in enumerate(runs)]
    keys = []
    for r in runs:
        for row in r:
            k = (row['cell'], row['B'], row['T'], row['fs'])
            if k not in keys:
                keys.append(k)
    keys.sort()
    print('median microseconds per call on device events (S = 1024); runs in the order they were taken: ' + ', '.join(names))
    for what, col in (('front forward', 'fwd_us'), ('front backward', 'bwd_us'), ('Generator.generate, u = 1', 'gen_us')):
        print('\n%s' % what)
        print('%-5s %3s %4s %4s  ' % ('cell', 'B', 'T', 'fs') + ' '.join('%16s' % n for n in names))
        for k in keys:
            cells = []
            for r in runs:
                m = [row for row in r if (row['cell'], row['B'], row['T'], row['fs']) == k]
                cells.append('%16s' % ('%.1f%s' % (m[0][col], ' p' if m[0]['persistent'] else ' f') if m else '-'))
            print('%-5s %3d %4d %4d  ' % k + ' '.join(cells))
    print('\n(p = the persistent launches ran, f = the per-frame path)')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--json', default=None)
    ap.add_argument('--root', default=None)
    ap.add_argument('--tag', default='run')
    ap.add_argument('--cells', default='lstm,gru')
    ap.add_argument('--fs', default='200,256')
    ap.add_argument('--B', default='32,64')
    ap.add_argument('--T', default='41,200')
    ap.add_argument('--window', type=float, default=0.4)
    ap.add_argument('--table', nargs='+', default=None)
    a = ap.parse_args()
    if a.table:
        return table(a.table)
    assert a.json, '--json OUT.json'
    measure(a)


if __name__ == '__main__':
    main()
