"""Records which audiogan_amd.kernels functions the generator fronts call, in order, on the CPU kernel model.

  ROUTES            every route of GFrontFn, GRUFrontFn and front_sample, by name
  record(mp, r, T)  one forward + backward (or one front_sample) of route r at T frames -> [[K name, [argument summary]], ...]

The persistent launches have no CPU model that the routing could depend on: here each one is a stand-in that zero-fills its
outputs, put in place the way the ``routed`` fixture of test_front_stack.py puts the stacked one, with its predicate answering
True.  What a call is summarised to: a tensor by its shape, a list by its elements, None, and numbers / bools / strings by value.

tests/golden/launch_sequences.json holds what this recorder saw BEFORE the launch layer was reorganised (written by
``python -m tests.launch_recorder`` at that commit); tests/test_launch_layer.py compares.  It is never rewritten from the code
under test."""
import json
import os

import torch

from tests import kernel_model

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'launch_sequences.json')
B, FZ = 2, 16
FRAMES = (3, 0)

# route -> (front kind, layers, what runs, the predicates that answer True[, frame size[, state size]]).  Frame size 16 lets the
# one-layer backward take its fused two-launches-per-frame form (K.lstm_front_bwd_ok), which frame size 8 never reaches; state
# size 36 is refused by K.lstm_step_ok and K.skinny_ok: the forward steps as GEMM + pointwise launches
ROUTES = {
    'lstm1_frames': ('lstm', 1, 'train', ()),
    'lstm1_launch': ('lstm', 1, 'train', ('gfront_persist_ok', 'gfront_bwd_persist_ok')),
    'lstm1_frames_fs16': ('lstm', 1, 'train', (), 16),
    'lstm2_frames': ('lstm', 2, 'train', ()),
    'lstm2_frames_s36': ('lstm', 2, 'train', (), 8, 36),
    'lstm2_launch': ('lstm', 2, 'train', ('gfront_stack_ok', 'gfront_stack_bwd_ok')),
    'gru_frames': ('gru', 1, 'train', ()),
    'gru_launch': ('gru', 1, 'train', ('gfront_persist_ok', 'gfront_bwd_persist_ok')),
    'sample_lstm2_stack': ('lstm', 2, 'sample', ('gfront_stack_ok',)),
    'sample_lstm1_launch': ('lstm', 1, 'sample', ('gfront_persist_ok',)),
    'sample_gru_launch': ('gru', 1, 'sample', ('gfront_persist_ok',)),
    'sample_lstm1_frames': ('lstm', 1, 'sample', ()),
    'sample_lstm2_frames': ('lstm', 2, 'sample', ()),
    'sample_gru_frames': ('gru', 1, 'sample', ()),
}

# the outputs each stand-in launch zero-fills, by argument name
_LAUNCHES = {
    'gfront_fwd_persist': ('gates wx whh wp bp hs cs x xt', 'hs cs x xt'),
    'gfront_bwd_persist': ('gates cs x dh_ext dx_ext whh wx wp dgs dxt', 'dgs dxt'),
    'grufront_fwd_persist': ('gates gh wx whh bhn wp bp hs x xt', 'gh hs x xt'),
    'grufront_bwd_persist': ('gates hs gh x dh_ext dx_ext whh wx wp dgi dgh dxt', 'dgi dgh dxt'),
    'gfront_gen_persist': ('pre wx whh wp bp ws bs u x s first t_run bhn', 'x s first t_run'),
    'gfront_stack_fwd_persist': ('gates wx w_in whh bias wp bp hs cs x xt', 'gates hs cs x xt'),
    'gfront_stack_gen_persist': ('pre wx w_in whh bias wp bp ws bs u x s first t_run', 'x s first t_run'),
    'gfront_stack_bwd_persist': ('gates cs x dh_ext dx_ext whh w_in wx wp dgs dxt', 'dgs dxt'),
}
_PREDICATES = ('gfront_persist_ok', 'gfront_bwd_persist_ok', 'gfront_stack_ok', 'gfront_stack_bwd_ok')


def _stand_in(names, outs):
    names, outs = names.split(), outs.split()

    def launch(*a, **k):
        args = dict(zip(names, a), **k)
        for n in outs:
            for t in (args.get(n) if isinstance(args.get(n), (list, tuple)) else [args.get(n)]):
                if t is not None:
                    t.zero_()
    return launch


def _summary(v):
    if isinstance(v, torch.Tensor):
        return list(v.shape)
    if isinstance(v, (list, tuple)):
        return [_summary(e) for e in v]
    if v is None or isinstance(v, (bool, int, float, str)):
        return v
    return type(v).__name__


def _inputs(kind, nl, T, FS, S):
    gen = torch.Generator().manual_seed(77)
    G = 3 if kind == 'gru' else 4
    shapes = []
    for l in range(nl):
        shapes += [(G * S, FS + FZ if l == 0 else S), (G * S, S), (G * S,), (G * S,)]
    shapes += [(FS, S), (FS,), (1, S), (1,)]
    vg = []
    for shp in shapes:
        v = torch.randn(shp, generator=gen) / (shp[-1] ** 0.5 if len(shp) > 1 else 4.0)
        nrm = v.reshape(shp[0], -1).norm(dim=1) if len(shp) > 1 else v.abs()
        vg.append((v, nrm.view([shp[0]] + [1] * (len(shp) - 1)).clone()))
    return vg, torch.randn(T, B, FZ, generator=gen), torch.rand(T, B, generator=gen)


def record(monkeypatch, route, T):
    """the calls of one route at T frames; ``monkeypatch``: pytest's (everything it sets is undone by the caller's fixture)"""
    import audiogan_amd.kernels as K
    from audiogan_amd import ops, recurrent
    kind, nl, what, on = ROUTES[route][:4]
    FS, S = (ROUTES[route][4:] + (8, 32)[len(ROUTES[route]) - 4:])
    kernel_model.install(monkeypatch)
    for n, (names, outs) in _LAUNCHES.items():
        monkeypatch.setattr(K, n, _stand_in(names, outs))
    for n in _PREDICATES:
        monkeypatch.setattr(K, n, (lambda *a_, _v=n in on: _v))
    calls = []

    def spy(n, fn):
        def f(*a, **k):
            calls.append([n, [_summary(v) for v in a] + [[q, _summary(k[q])] for q in sorted(k)]])
            return fn(*a, **k)
        return f
    for n in sorted(set(kernel_model.ALL) | set(_LAUNCHES)):
        fn = getattr(K, n)
        if n != 'install' and not n.endswith('_ok') and not isinstance(fn, type):
            monkeypatch.setattr(K, n, spy(n, fn))
    vg, zc, u = _inputs(kind, nl, T, FS, S)
    front = ops.GRUFront(FS, S) if kind == 'gru' else ops.GFront(FS, nl, S)
    for v, g in vg:
        front.group.add(torch.nn.Parameter(v), torch.nn.Parameter(g))
    try:
        if what == 'sample':
            with torch.no_grad():
                recurrent.front_sample(front, zc, u)
            return calls
        zc.requires_grad_(True)
        x, s = (ops.GRUFrontFn if kind == 'gru' else ops.GFrontFn).apply(zc, front, *front.group.params())
        calls.append(['backward', []])
        (x.sum() + s.sum()).backward()
    except Exception as e:      # (an empty sequence that torch refuses downstream of the launches: part of the record)
        calls.append(['raised', [type(e).__name__]])
    return calls


def record_all(monkeypatch_factory):
    out = {}
    for route in ROUTES:
        for T in FRAMES:
            with monkeypatch_factory() as mp:
                out['%s/T%d' % (route, T)] = record(mp, route, T)
    return out


if __name__ == '__main__':
    import pytest
    with open(GOLDEN, 'w') as f:
        json.dump(record_all(pytest.MonkeyPatch.context), f, separators=(',', ':'))
        f.write('\n')
    print('wrote', GOLDEN)
