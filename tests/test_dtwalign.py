"""Word cuts by template alignment on the CPU: the model of kernels.dtw_align (tests/dtwalign_model.py) against
align.path64 and against the definition of a path, the mutants the checkers must reject, ag_dtw_align's refusals (host code,
no GPU), align.reference_for / medoid / pick_templates, the two transcript readers, and the tool end to end on the kernel
models.  The GPU half is tests/test_gpu_dtwalign.py.

Bounds: the module text of tests/dtwalign_model.py."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from audiogan_amd import align, audio, ingest
from tests import align_model, dtwalign_model as M, eval_model, kernel_model, pairs_model


def _models(monkeypatch):
    kernel_model.install(monkeypatch)
    eval_model.install(monkeypatch)
    align_model.install(monkeypatch)
    pairs_model.install(monkeypatch)
    M.install(monkeypatch)
    monkeypatch.setattr(align, 'require_device', lambda device: torch.device('cpu'))


# ------------------------------------------------------------------------------------------------------------------
# the model under its checkers
# ------------------------------------------------------------------------------------------------------------------
def test_model_equals_path64_on_the_integer_cases():
    for case in (M.SMALL, M.GRID, M.CLAMP, M.LIMIT):
        M.check_exact(M.dtw_align, case, 'integer')
    M.check_exact(M.dtw_align, M.EQUAL, 'equal')


def test_all_equal_pair_pins_the_tie_order():
    """every cell ties three ways: the diagonal while there is one, then up in column 0 or left on row 0"""
    _, lo, hi = M.check_exact(M.dtw_align, M.EQUAL, 'equal')
    assert lo[0, :3].tolist() == [0, 3, 4] and hi[0, :3].tolist() == [2, 3, 4]                      # (5, 3)
    assert lo[1, :5].tolist() == [0, 0, 0, 1, 2] and hi[1, :5].tolist() == [0, 0, 0, 1, 2]          # (3, 5)
    assert lo[2, :4].tolist() == [0, 1, 2, 3] and hi[2, :4].tolist() == [0, 1, 2, 3]                # (4, 4)
    assert lo[3, :4].tolist() == [0, 0, 0, 0] and hi[4, :1].tolist() == [3]                         # one row; one column
    total, lo64, hi64 = align.path64(np.zeros((5, 16)), 5, np.zeros((3, 16)), 3)
    assert total == 0.0 and lo64.tolist() == [0, 3, 4] and hi64.tolist() == [2, 3, 4]


def test_path_facts_and_path_cost_on_real_cases():
    for case in (M.SMALL, M.GRID, M.CLAMP):
        ratio = M.check_real(M.dtw_align, case, cost_fn=align_model.dtw_cost)
        print('dtw_align model, real pass: largest (cost of the returned path - D64) / bound %.3e' % ratio)


@pytest.mark.parametrize('mutant,case,kind', [
    ('tie_swapped', M.EQUAL, 'equal'),                 # the all-equal pairs: the path IS the tie order
    ('lohi_off_by_one', M.SMALL, 'integer'),           # (7, 5): a column left from a row that is not its last
    ('diag1', M.SMALL, 'integer'),                     # (2, 2) on: the diagonal at weight 1 undercuts the total
    ('unclamped', M.CLAMP, 'integer'),                 # a count of 0 is one frame
])
def test_checker_rejects_mutants(mutant, case, kind):
    with pytest.raises(AssertionError):
        M.check_exact(M.dtw_align, case, kind, mutate=mutant)
    M.check_exact(M.dtw_align, case, kind)          # (the same case without the mutation passes)


# ------------------------------------------------------------------------------------------------------------------
# the launcher's refusals
# ------------------------------------------------------------------------------------------------------------------
_HOST = ctypes.create_string_buffer(64 + 16)
PTR = (ctypes.addressof(_HOST) + 15) & ~15


def test_launcher_refuses_before_any_hip_call():
    """every refusal of ag_dtw_align: AG_ERR_ARG from host code, with no device in sight (the pointers are host memory: a
    launch would not survive them)"""
    import audiogan_amd.kernels as K
    from audiogan_amd import _lib
    p = ctypes.c_void_p(PTR)
    assert K.dtw_align_ws(1024, 1024) == 256 * 1024 and K.dtw_align_ws(8, 17) == 8 * 2 * 4 and K.dtw_align_ws(1, 1) == 4
    assert K.dtw_align_ws(0, 8) == K.dtw_align_ws(8, 1025) == 0
    ok = dict(ca=p, na=p, cb=p, nb=p, total=p, lo=p, hi=p, ws=p, bytes=3 * 8 * 2 * 4, B=3, Fa=8, Fb=17)

    def call(**bad):
        a = dict(ok, **bad)
        return K.lib.ag_dtw_align(a['ca'], a['na'], a['cb'], a['nb'], a['total'], a['lo'], a['hi'], a['ws'], a['bytes'], a['B'],
                                  a['Fa'], a['Fb'], None)
    for bad in (dict(ca=None), dict(cb=None), dict(total=None), dict(lo=None), dict(hi=None), dict(ws=None), dict(B=0),
                dict(B=-2), dict(Fa=0), dict(Fb=0), dict(Fa=1025), dict(Fb=1025), dict(bytes=3 * 8 * 2 * 4 - 1), dict(bytes=0),
                dict(B=4), dict(Fb=33)):
        assert call(**bad) == _lib.AG_ERR_ARG, bad
        assert K.lib.ag_last_error().startswith(b'ag_dtw_align'), bad
    assert call(Fa=1025) == _lib.AG_ERR_ARG and b'1024' in K.lib.ag_last_error()
    # the wrapper: a CPU tensor, a wrong dtype, a wrong shape, each named
    z = torch.zeros(2, 4, 16)
    with pytest.raises(RuntimeError, match='cep_a must be a CUDA'):
        K.dtw_align(z, None, z, None)


# ------------------------------------------------------------------------------------------------------------------
# references and templates
# ------------------------------------------------------------------------------------------------------------------
def test_reference_layout_and_the_pause_column():
    rs = np.random.RandomState(3)
    templates = {w: rs.randn(k, 16).astype(np.float32) for w, k in (('a', 3), ('b', 1), ('c', 5))}
    cep = rs.randn(25, 16).astype(np.float32)
    cep[:, 0] = [5, 9, -7, 4, 8, 3, -7, 6, 2, 7] + [10 + k for k in range(15)]          # hand-written c[0]
    # 25 frames: the lowest tenth is 2 frames - rows 2 and 6 (both -7)
    sil = align.pause_frame(cep)
    assert sil.dtype == np.float32 and np.array_equal(sil, cep[[2, 6]].astype(np.float64).mean(0).astype(np.float32))
    # a count: only the first 9 frames -> one frame, the first of the two equal ones
    assert np.array_equal(align.pause_frame(cep, 9), cep[2])
    assert np.array_equal(align.pause_frame(cep[:1]), cep[0])          # at least one frame
    ref, offsets, lengths = align.reference_for(['c', 'a', 'a', 'b'], templates, cep)
    assert offsets == [1, 7, 11, 15] and lengths == [5, 3, 3, 1] and ref.shape == (17, 16) and ref.dtype == np.float32
    assert align.reference_frames(['c', 'a', 'a', 'b'], templates) == 17
    for col in (0, 6, 10, 14, 16):
        assert np.array_equal(ref[col], sil), col
    assert np.array_equal(ref[1:6], templates['c']) and np.array_equal(ref[7:10], templates['a'])
    assert np.array_equal(ref[11:14], templates['a']) and np.array_equal(ref[15:16], templates['b'])
    # the cut of a word: first frame of its first column to the end of the last frame of its last column
    lo, hi = np.arange(17) * 2, np.arange(17) * 2 + 1
    assert align.word_span(lo, hi, 7, 3, 10 ** 6) == (14 * 128, 19 * 128 + 256)
    assert align.word_span(lo, hi, 15, 1, 4000) == (30 * 128, 4000)


def test_medoid_and_its_tie():
    M3 = np.array([[0.0, 4.0, 6.0], [4.0, 0.0, 1.0], [6.0, 1.0, 0.0]])
    assert align.medoid(M3) == 1
    tie = np.array([[0.0, 2.0, 5.0, 3.0], [2.0, 0.0, 4.0, 1.0], [5.0, 4.0, 0.0, 1.0], [3.0, 1.0, 1.0, 0.0]])
    assert tie.sum(1).tolist() == [10.0, 7.0, 10.0, 5.0] and align.medoid(tie) == 3
    tie[3, :] = tie[:, 3] = [3.0, 2.0, 2.0, 0.0]
    tie[1, 2] = tie[2, 1] = 3.0          # sums 10, 7, 10, 7: rows 1 and 3 are equally central
    assert tie.sum(1)[1] == tie.sum(1)[3] == 7.0 and align.medoid(tie) == 1          # the lowest index
    assert align.medoid(np.zeros((1, 1))) == 0


def test_pick_templates_on_the_models(monkeypatch):
    _models(monkeypatch)
    import audiogan_amd.kernels as K
    store = M.template_store()
    a, far = store['alpha'][0], store['echo'][0]
    near = M.burst('alpha', 1.1).astype(np.float32)
    clips = np.zeros((4, max(len(a), len(far), len(near))), dtype=np.float32)
    for r, c in enumerate((far, a, near, far[::-1].copy())):          # the fourth clip is past per_word=3
        clips[r, :len(c)] = c
    got = align.pick_templates(dict(alpha=clips, bravo=store['bravo']), ['bravo', 'alpha', 'golf', 'alpha'], per_word=3)
    assert sorted(got) == ['alpha', 'bravo']
    lens = torch.tensor([len(far), len(a), len(near)])
    nf = torch.empty(3, dtype=torch.int32)
    cep = K.melcep_frames(torch.from_numpy(clips[:3]), lens, nframes=nf)
    D = (K.dtw_pairs(cep, nf, cep, nf).double() / (nf[:, None] + nf[None, :]).double()).numpy()
    pick = align.medoid(D)
    assert pick in (1, 2)          # one of the two takes of the word, not the other word's clip
    assert np.array_equal(got['alpha'], cep[pick, :int(nf[pick])].numpy())
    own = K.melcep_frames(torch.from_numpy(store['bravo']), torch.tensor([store['bravo'].shape[1]]))
    assert np.array_equal(got['bravo'], own[0].numpy())          # one clip: its own template
    assert align.pick_templates(store, ['golf']) == {}


# ------------------------------------------------------------------------------------------------------------------
# readers
# ------------------------------------------------------------------------------------------------------------------
def test_read_utterances(tmp_path):
    tsv = os.path.join(tmp_path, 'u.tsv')
    with open(tsv, 'wb') as f:
        f.write(b'# path, start, end, transcript, channel\n\n'
                b'a.wav\t0.5\t2.25\tone two  three\n'
                b'/abs/b.wav\t\t\tfour\t1   # a comment\r\n'
                b'sub/c.wav\t1\t2\tfive six\t0\n')
    got = ingest.read_utterances(tsv)
    here = str(tmp_path)
    assert got == [(os.path.join(here, 'a.wav'), 0.5, 2.25, ['one', 'two', 'three'], None),
                   ('/abs/b.wav', None, None, ['four'], 1),
                   (os.path.join(here, 'sub/c.wav'), 1.0, 2.0, ['five', 'six'], 0)]
    with open(tsv, 'wb') as f:
        f.write(b'a.wav\tone two\n')
    with pytest.raises(ValueError, match='u.tsv:1'):
        ingest.read_utterances(tsv)


def test_read_fisher_transcript(tmp_path):
    txt = os.path.join(tmp_path, 'fe_03_00001.txt')
    with open(txt, 'wb') as f:
        f.write(b'# fe_03_00001.sph\n# Transcribed at the LDC\n\n'
                b'0.45 1.32 A: Hello there\n'
                b'1.10 2.96 B: hi [laughter] how ARE you\n'
                b'3.02 3.50 A: (( mumble mumble )) fine\n'
                b'3.60 4.10 B: [noise]\n'
                b'4.2 x A: not a time\n'
                b'5.00 6.00 C: no such channel\n'
                b'6.00 7.50 B-f: well ((you)) know\n')
    got = ingest.read_fisher_transcript(txt, '/data/fe_03_00001.wav')
    assert got == [('/data/fe_03_00001.wav', 0.45, 1.32, ['hello', 'there'], 0),
                   ('/data/fe_03_00001.wav', 1.10, 2.96, ['hi', 'how', 'are', 'you'], 1),
                   ('/data/fe_03_00001.wav', 3.02, 3.50, ['fine'], 0),
                   ('/data/fe_03_00001.wav', 6.00, 7.50, ['well', 'know'], 1)]


# ------------------------------------------------------------------------------------------------------------------
# the tool, end to end on the models
# ------------------------------------------------------------------------------------------------------------------
def write_utterance_files(tmp_path):
    """the synthetic utterances as 8 kHz float WAV files, a template store, and the TSV: whole files and one bounded entry
    -> (tsv, templates.npz, truth)"""
    waves, lens, transcripts, truth = M.utterances()
    lines = []
    for u in range(len(lens)):
        path = os.path.join(tmp_path, 'utt%d.wav' % u)
        audio.write_wav(path, waves[u, :lens[u]], sr=M.SR)
        bounds = '\t' if u != 1 else '%.6f\t%.6f' % (0.0, (lens[u] + 0.5) / M.SR)
        lines.append('utt%d.wav\t%s\t%s\n' % (u, bounds, ' '.join(transcripts[u])))
    tsv = os.path.join(tmp_path, 'utterances.tsv')
    with open(tsv, 'w') as f:
        f.writelines(lines)
    npz = os.path.join(tmp_path, 'templates.npz')
    ingest.save_store(M.template_store(), npz)
    return tsv, npz, truth


def check_cuts_against_truth(report, truth, transcripts):
    """every word cut, in order, every boundary within BOUNDARY_TOLERANCE frames -> the largest error in frames"""
    cuts = report['cuts']
    assert [w for _, w, _, _, _ in cuts] == [w for words in transcripts for w in words]
    flat = [span for spans in truth for span in spans]
    worst = 0.0
    for (_, w, a, z, db), (s, e) in zip(cuts, flat):
        worst = max(worst, abs(a - s) / 128.0, abs(z - e) / 128.0)
        assert np.isfinite(db) and db >= 0.0
    assert worst <= M.BOUNDARY_TOLERANCE, worst
    return worst


def test_the_arbiters_own_boundary_error_is_the_documented_one():
    out, truth = M.cuts64()
    assert M.boundary_errors(out, truth) == M.PATH64_WORST == 1.625 and M.BOUNDARY_TOLERANCE == 2.625


def test_tool_end_to_end_on_the_models(monkeypatch, tmp_path, capsys):
    _models(monkeypatch)
    tsv, npz, truth = write_utterance_files(tmp_path)
    _, _, transcripts, _ = M.utterances()
    utts = ingest.read_utterances(tsv)
    templates = align.pick_templates(ingest.load_store(npz), [w for u in utts for w in u[3]])
    assert sorted(templates) == sorted(M.WORDS)
    store, report = ingest.align_store(utts, templates)
    worst = check_cuts_against_truth(report, truth, transcripts)
    print('align_store on the models: largest boundary error %.3f frames (path64 on float64 cepstra %.3f, tolerance %.3f)'
          % (worst, M.PATH64_WORST, M.BOUNDARY_TOLERANCE))
    counts = {}
    for words in transcripts:
        for w in words:
            counts[w] = counts.get(w, 0) + 1
    assert report['kept'] == counts and not any(report['dropped'].values()) and report['files'] == 4
    assert sorted(report['dropped']) == sorted(ingest.DROPPED)
    # the command line: the same store; --cuts-out, then --manifest: the same store again, bit for bit
    out, cuts, back = (os.path.join(tmp_path, n) for n in ('words2.npz', 'cuts.tsv', 'back.npz'))
    assert ingest.main(['--utterances', tsv, '--templates', npz, '--out', out, '--cuts-out', cuts]) == 0
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line['kept'] == counts and line['missing_words'] == {} and line['dropped']['no_template'] == 0
    assert ingest.main(['--manifest', cuts, '--out', back, '--device', 'cpu']) == 0
    a, b, c = ingest.load_store(out), ingest.load_store(back), store
    assert list(a) == list(b) == list(c)
    for w in a:
        assert a[w].dtype == b[w].dtype == np.float32 and np.array_equal(a[w], b[w]) and np.array_equal(a[w], c[w]), w
    assert len(ingest.read_manifest(cuts)) == sum(counts.values())
    # --trim narrows cuts and never widens them; --max-db 0 drops every cut as poor_match (no take equals its template)
    _, trimmed = ingest.align_store(utts, templates, trim=True)
    assert len(trimmed['cuts']) == len(report['cuts'])
    assert all(t[2] >= r[2] and t[3] <= r[3] for t, r in zip(trimmed['cuts'], report['cuts']))
    none, rep = ingest.align_store(utts, templates, max_db=0.0)
    assert none == {} and len(rep['dropped']['poor_match']) == sum(counts.values())


def test_drops_are_reported_not_raised(monkeypatch, tmp_path):
    _models(monkeypatch)
    tsv, npz, _ = write_utterance_files(tmp_path)
    long_wav, broken = os.path.join(tmp_path, 'long.wav'), os.path.join(tmp_path, 'broken.wav')
    audio.write_wav(long_wav, np.random.RandomState(0).randn(1025 * 128 + 256).astype(np.float32) * 0.01, sr=M.SR)
    with open(broken, 'wb') as f:
        f.write(b'RIFFnope')
    utts = ingest.read_utterances(tsv)[:1] + [
        (os.path.join(tmp_path, 'utt1.wav'), None, None, ['delta', 'golf', 'alpha', 'hotel', 'golf'], None),
        (long_wav, None, None, ['alpha'], None), (broken, None, None, ['alpha'], None),
        (os.path.join(tmp_path, 'utt0.wav'), None, None, ['alpha'], 1)]          # a channel the file does not have
    templates = align.pick_templates(ingest.load_store(npz), list(M.WORDS))
    store, report = ingest.align_store(utts, templates)
    assert report['kept'] == dict(alpha=1, bravo=1, coda=1)
    assert report['dropped']['no_template'] == [utts[1][0]] and report['missing_words'] == dict(golf=1, hotel=1)
    assert report['dropped']['too_long_to_align'] == [long_wav]
    assert report['dropped']['unreadable'] == [broken, utts[4][0]]
    # a reference past 1024 frames: 60 words of 18 frames and up
    res = align.align_utterances(np.zeros((1, 4000), dtype=np.float32), [4000], [['coda'] * 60], templates)
    assert res[0]['dropped'][0] == 'too_long_to_align' and res[0]['cuts'] == []


def test_the_tool_says_that_it_needs_a_device(tmp_path, capsys):
    tsv, npz, _ = write_utterance_files(tmp_path)
    out = os.path.join(tmp_path, 'never.npz')
    assert ingest.main(['--utterances', tsv, '--templates', npz, '--out', out, '--device', 'cpu']) == 2
    assert 'CUDA (HIP) device' in capsys.readouterr().err and not os.path.exists(out)
    with pytest.raises(RuntimeError, match='CUDA'):
        align.align_utterances(np.zeros((1, 300), dtype=np.float32), [300], [['alpha']], {}, device='cpu')
    with pytest.raises(SystemExit):
        ingest.main(['--utterances', tsv, '--out', out])          # no --templates
    with pytest.raises(SystemExit):
        ingest.main(['--manifest', tsv, '--templates', npz, '--out', out])
