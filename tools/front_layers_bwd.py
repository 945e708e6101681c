"""The backward through time of a STACKED LSTM front (Generator(num_layers=nl)) in one persistent launch
(ag_gfront_stack_bwd) against the per-frame chain (K.PERSIST_FRONT_STACK_BWD[0] = False: one launch per operation and frame,
for these shapes the code of the commit before the launch existed), on HIP events, S = 1024: per (nl, fs, B, T)

    fwd_bwd    forward + backward of the front (the forward is the stacked launch in both columns)
    bwd        the backward alone: the events sit around autograd's backward of a forward that ran before them (the stop head's
               gradients, the frame loop, the weight-gradient GEMMs over all frames, the weight-norm backward)

    python tools/front_layers_bwd.py [--json OUT.json] [--nl 2] [--fs 200] [--B 32] [--T 41,200] [--rounds 4]

Every shape is warmed in both modes first; then ``--rounds`` alternating rounds (one launch, per-frame, one launch, ...) in ONE
process, each figure the median of repetitions covering about ``--window`` seconds of device time.  The gate of the launch's
default (README): its median is below the per-frame one's in EVERY round at every T, for both figures.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _time(fn, window, lo=5, hi=300):
    """fn() -> (e0, e1) recorded around what is measured"""
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    ts = []
    while len(ts) < lo or (sum(ts) < window * 1e6 and len(ts) < hi):
        e0, e1 = fn()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    ts.sort()
    return ts[len(ts) // 2]


def _setup(A, K, ops, nl, fs, B, T, dev):
    S, ns, es = 1024, 100, 100
    torch.manual_seed(0)
    g = A.Generator(num_layers=nl, frame_size=fs, embed_size=es, noise_size=ns, state_size=S).to(dev)
    assert K.gfront_stack_bwd_ok(B, S, fs, nl, dev), 'this shape does not take the one-launch backward on this device'
    z, c = torch.randn(B, T, ns, device=dev), torch.randn(B, es, device=dev)
    zc = ops.BuildZCFn.apply(z, c)
    gx, gs = torch.randn(B, T * fs, device=dev), torch.randn(B, T, device=dev)
    g.refresh_weights()
    ev = lambda: torch.cuda.Event(enable_timing=True)      # noqa: E731

    def fwd_bwd():
        e0, e1 = ev(), ev()
        e0.record()
        xs = g._front_apply(zc)
        torch.autograd.backward(list(xs), [gx, gs])
        e1.record()
        return e0, e1

    def bwd():
        e0, e1 = ev(), ev()
        xs = g._front_apply(zc)
        e0.record()
        torch.autograd.backward(list(xs), [gx, gs])
        e1.record()
        return e0, e1
    return g, [('fwd_bwd', fwd_bwd), ('bwd', bwd)]


def measure(a):
    import audiogan_amd as A
    from audiogan_amd import kernels as K, ops
    dev = torch.device('cuda')
    K.lstm_persist_status(reset=True)
    default = K.PERSIST_FRONT_STACK_BWD[0]
    rows = []
    shapes = [(nl, fs, B, T) for nl in a.nl for fs in a.fs for B in a.B for T in a.T]
    sets = {sh: _setup(A, K, ops, *sh, dev) for sh in shapes}
    for sh in shapes:                                   # every shape warmed in both modes
        for on in (True, False):
            K.PERSIST_FRONT_STACK_BWD[0] = on
            for _, fn in sets[sh][1]:
                fn()
    torch.cuda.synchronize()
    for rnd in range(a.rounds):
        for on in (True, False):
            K.PERSIST_FRONT_STACK_BWD[0] = on
            for sh in shapes:
                g, fns = sets[sh]
                row = dict(round=rnd + 1, mode='one-launch' if on else 'per-frame', nl=sh[0], fs=sh[1], B=sh[2], T=sh[3])
                for name, fn in fns:
                    row[name + '_us'] = _time(fn, a.window)
                    for q in g.parameters():
                        q.grad = None
                rows.append(row)
                print('round %d  %-10s nl %d fs %3d B %2d T %3d   fwd_bwd %9.1f   bwd %9.1f us'
                      % (rnd + 1, row['mode'], sh[0], sh[1], sh[2], sh[3], row['fwd_bwd_us'], row['bwd_us']), flush=True)
    K.PERSIST_FRONT_STACK_BWD[0] = default
    torch.cuda.synchronize()
    assert K.lstm_persist_status() == 0, 'a persistent launch gave up'
    gate = True
    for sh in shapes:
        for rnd in range(a.rounds):
            for key in ('fwd_bwd_us', 'bwd_us'):
                t = {r['mode']: r[key] for r in rows if (r['nl'], r['fs'], r['B'], r['T']) == sh and r['round'] == rnd + 1}
                gate = gate and t['one-launch'] < t['per-frame']
    print('gate (the one-launch backward below the per-frame chain in every round at every shape): %s' % ('PASS' if gate else 'FAIL'))
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(dict(rows=rows, gate=gate), f, indent=1)


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
    measure(ap.parse_args())


if __name__ == '__main__':
    main()
