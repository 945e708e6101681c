"""Generator.generate at the C2 widths (B = 64, S = 1024, fs = 256, T = 32) on HIP events: the frames the sampling loop ran
(t_run) and the time of the front alone (the z/c pre-activation GEMM + the ag_gfront_fwd launch (gen = 1)), for three kinds of
stop uniforms u:

    never    u = 1: no clip stops, all 32 frames run
    natural  u ~ U(0,1) against a fresh generator's stop head (p ~ 0.5 per frame)
    forced8  u = 0 at frame 8 for every clip (first = 9 frames), 1 elsewhere

plus, for scale, the training front's persistent forward over all 32 frames (which also writes the gate / state history)
and the whole generate call (front + the one host read + the conv trunk on the kept frames).

    python tools/prof_generate.py [--iters N] [--json PATH]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _time(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    ts.sort()
    return ts[len(ts) // 2], ts[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    import audiogan_amd as A
    from audiogan_amd import kernels as K, ops
    from audiogan_amd.recurrent import front_sample
    dev = torch.device('cuda')
    B, S, fs, T, ns, es = 64, 1024, 256, 32, 100, 100
    torch.manual_seed(0)
    g = A.Generator(frame_size=fs, embed_size=es, noise_size=ns, state_size=S, num_layers=1).to(dev)
    assert g.front_is_persistent(B, dev)
    z, c = torch.randn(B, T, ns, device=dev), torch.randn(B, es, device=dev)
    zc = ops.BuildZCFn.apply(z, c)
    g.refresh_weights()
    u_never = torch.ones(T, B, device=dev)
    u_nat = torch.rand(T, B, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    u_8 = torch.ones(T, B, device=dev)
    u_8[8] = 0.0
    K.lstm_persist_status(reset=True)
    rows = []
    with torch.no_grad():
        med, best = _time(lambda: g._front_apply(zc), a.iters)
        rows.append(dict(case='training front (32 frames, history)', t_run=T, front_us=med, front_us_min=best))
        for name, u in (('never', u_never), ('natural', u_nat), ('forced8', u_8)):
            _, _, first, t_run = front_sample(g._front, zc, u)
            torch.cuda.synchronize()
            med, best = _time(lambda: front_sample(g._front, zc, u), a.iters)
            gmed, _ = _time(lambda: g.generate(c, z=z, u=u), max(5, a.iters // 5))
            rows.append(dict(case=name, t_run=int(t_run), t_eff=int(first.max()), front_us=med, front_us_min=best,
                             generate_us=gmed))
    torch.cuda.synchronize()
    assert K.lstm_persist_status() == 0, 'a persistent launch gave up'
    for r in rows:
        print('%-38s t_run %2d  %s front %7.1f us (min %7.1f)%s' % (
            r['case'], r['t_run'], ('t_eff %2d ' % r['t_eff']) if 't_eff' in r else ' ' * 9, r['front_us'], r['front_us_min'],
            ('  generate %8.1f us' % r['generate_us']) if 'generate_us' in r else ''))
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(rows, f, indent=1)


if __name__ == '__main__':
    main()
