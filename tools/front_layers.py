"""The STACKED LSTM front (Generator(num_layers=nl)) in one persistent launch (ag_gfront_stack_fwd) against the per-frame path
(K.PERSIST_FRONT_STACK[0] = False: one launch per operation and frame, for these shapes the code of the commit before the
launch existed), on HIP events, S = 1024: per (nl, fs, B, T)

    fwd        the training forward of the front (the z/c pre-activation GEMM, the frame loop, the stop head)
    gen_all    Generator.generate with u = 1 (no clip stops: all T frames, the conv trunk on all of them)
    gen_stop5  Generator.generate with the last stop drawn at frame 5 (the stacked launch leaves its loop after 6 + lag frames;
               the per-frame path runs all T frames of the front, the trunk runs on 6 frames either way)
    fwd_bwd    forward + backward of the front (the backward is the per-frame chain in both columns: the baseline a one-launch
               stacked backward will be measured against)

    python tools/front_layers.py [--json OUT.json] [--nl 2] [--fs 200] [--B 32] [--T 41,200] [--rounds 4]
    python tools/front_layers.py --trace N [--per-frame]     N forwards + generates (u = 1) of one mode only, for a
                                                             rocprofv3 --kernel-trace --stats run of its own

Every shape is warmed in both modes first; then ``--rounds`` alternating rounds (stacked, per-frame, stacked, ...) in ONE
process, each figure the median of repetitions covering about ``--window`` seconds of device time.  The gate of the launch's
default (README): the stacked forward's median is below the per-frame one's in EVERY round at every T.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _time(fn, window, lo=5, hi=300):
    for _ in range(2):
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
    return ts[len(ts) // 2]


def _setup(A, K, ops, nl, fs, B, T, dev):
    S, ns, es = 1024, 100, 100
    torch.manual_seed(0)
    g = A.Generator(num_layers=nl, frame_size=fs, embed_size=es, noise_size=ns, state_size=S).to(dev)
    assert K.gfront_stack_ok(B, S, fs, nl, dev), 'this shape does not take the stacked launch on this device'
    z, c = torch.randn(B, T, ns, device=dev), torch.randn(B, es, device=dev)
    zc = ops.BuildZCFn.apply(z, c)
    gx, gs = torch.randn(B, T * fs, device=dev), torch.randn(B, T, device=dev)
    u1 = torch.ones(T, B, device=dev)
    u5 = torch.ones(T, B, device=dev)
    if T > 5:
        u5[(5 - torch.arange(B)) % 6, torch.arange(B)] = 0.0          # clip b stops at frame (5 - b) % 6: the last at frame 5
    g.refresh_weights()

    def fwd():
        g._front_apply(zc)

    def fwd_bwd():
        xs = g._front_apply(zc)
        torch.autograd.backward(list(xs), [gx, gs])

    def gen_all():
        with torch.no_grad():
            g.generate(c, z=z, u=u1)

    def gen_stop5():
        with torch.no_grad():
            g.generate(c, z=z, u=u5)
    return g, [('fwd', fwd), ('gen_all', gen_all), ('gen_stop5', gen_stop5), ('fwd_bwd', fwd_bwd)]


def measure(a):
    import audiogan_amd as A
    from audiogan_amd import kernels as K, ops
    dev = torch.device('cuda')
    K.lstm_persist_status(reset=True)
    rows = []
    shapes = [(nl, fs, B, T) for nl in a.nl for fs in a.fs for B in a.B for T in a.T]
    sets = {sh: _setup(A, K, ops, *sh, dev) for sh in shapes}
    for sh in shapes:                                   # every shape warmed in both modes
        for on in (True, False):
            K.PERSIST_FRONT_STACK[0] = on
            for _, fn in sets[sh][1]:
                fn()
    torch.cuda.synchronize()
    for rnd in range(a.rounds):
        for on in (True, False):
            K.PERSIST_FRONT_STACK[0] = on
            for sh in shapes:
                g, fns = sets[sh]
                row = dict(round=rnd + 1, mode='stacked' if on else 'per-frame', nl=sh[0], fs=sh[1], B=sh[2], T=sh[3])
                for name, fn in fns:
                    row[name + '_us'] = _time(fn, a.window)
                    for q in g.parameters():
                        q.grad = None
                row['t_run_stop5'] = None if g.last_t_run is None else int(g.last_t_run)
                rows.append(row)
                print('round %d  %-9s nl %d fs %3d B %2d T %3d   fwd %9.1f   gen_all %9.1f   gen_stop5 %9.1f (t_run %s)   fwd_bwd %9.1f us'
                      % (rnd + 1, row['mode'], sh[0], sh[1], sh[2], sh[3], row['fwd_us'], row['gen_all_us'], row['gen_stop5_us'],
                         row['t_run_stop5'], row['fwd_bwd_us']), flush=True)
    K.PERSIST_FRONT_STACK[0] = True
    torch.cuda.synchronize()
    assert K.lstm_persist_status() == 0, 'a persistent launch gave up'
    gate = True
    for sh in shapes:
        for rnd in range(a.rounds):
            t = {r['mode']: r['fwd_us'] for r in rows if (r['nl'], r['fs'], r['B'], r['T']) == sh and r['round'] == rnd + 1}
            gate = gate and t['stacked'] < t['per-frame']
    print('gate (stacked forward below the per-frame forward in every round at every shape): %s' % ('PASS' if gate else 'FAIL'))
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(dict(rows=rows, gate=gate), f, indent=1)


def trace(a):
    """one mode alone, a.trace times per shape: training forward and generate (u = 1)"""
    import audiogan_amd as A
    from audiogan_amd import kernels as K, ops
    dev = torch.device('cuda')
    for sh in [(nl, fs, B, T) for nl in a.nl for fs in a.fs for B in a.B for T in a.T]:
        g, fns = _setup(A, K, ops, *sh, dev)
        K.PERSIST_FRONT_STACK[0] = not a.per_frame
        fns = dict(fns)
        for _ in range(a.trace):
            fns['fwd']()
            fns['gen_all']()
    torch.cuda.synchronize()
    assert K.lstm_persist_status() == 0, 'a persistent launch gave up'


def main():
    ints = lambda s: [int(v) for v in s.split(',')]      # noqa: E731
    ap = argparse.ArgumentParser()
    ap.add_argument('--json', default=None)
    ap.add_argument('--nl', type=ints, default=[2])
    ap.add_argument('--fs', type=ints, default=[200])
    ap.add_argument('--B', type=ints, default=[32])
    ap.add_argument('--T', type=ints, default=[41, 200])
    ap.add_argument('--rounds', type=int, default=4)
    ap.add_argument('--window', type=float, default=0.25)
    ap.add_argument('--trace', type=int, default=0)
    ap.add_argument('--per-frame', action='store_true', help='--trace: the per-frame path instead of the stacked launch')
    a = ap.parse_args()
    if a.trace:
        return trace(a)
    measure(a)


if __name__ == '__main__':
    main()
