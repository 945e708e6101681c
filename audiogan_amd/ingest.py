"""From a folder of recordings to the word store the loader reads - what the reference's preprocessing scripts do with
``librosa.load(wav, sr=8000)``, a forced alignment and HDF5 (preprocess.py:24, preprocess-fisher.py:232-250), without
librosa, h5py or an alignment of its own: segments come from a manifest.

  scan_tree(root)        entries (path, word, None, None) for root/<word>/*.wav, sorted
  read_manifest(tsv)     entries from lines  path<TAB>word[<TAB>start_s<TAB>end_s]
  build_store(entries)   read (audio.read_wav), resample to 8 kHz (audio.resample: ag_resample_poly on a GPU, float64 on
                         the host otherwise), cut, drop, stack -> (store, report)
  save_store / load_store  one uncompressed .npz; ``dataset._open`` takes its path as ``args.dataset``

The store is a plain dict word -> float32 [n_clips, maxlen_word], zero padded: the layout preprocess-fisher.py:240-250
writes and dataset.py reads.  Samples are stored as resampled; the loader peak-normalises each pick, as the reference does.

  python -m audiogan_amd.ingest (--tree DIR | --manifest TSV) --out words.npz [--maxlen N] [--device D]"""
import argparse
import collections
import glob
import json
import os
import sys

import numpy as np

from . import audio

DROPPED = ('silent', 'too_long', 'unreadable')


def scan_tree(root):
    """entries (path, word, None, None) for root/<word>/*.wav, sorted by word, then by file name"""
    for word in sorted(os.listdir(root)):
        d = os.path.join(root, word)
        if os.path.isdir(d):
            for path in sorted(glob.glob(os.path.join(glob.escape(d), '*.wav'))):
                yield (path, word, None, None)


def read_manifest(tsv):
    """entries from lines ``path<TAB>word[<TAB>start_s<TAB>end_s]``; ``#`` starts a comment, empty lines are skipped and a
    relative path is taken from the manifest's directory"""
    here = os.path.dirname(os.path.abspath(tsv))
    out = []
    with open(tsv, encoding='utf-8') as f:
        for no, line in enumerate(f, 1):
            line = line.split('#', 1)[0].rstrip('\r\n')
            if not line.strip():
                continue
            cols = line.split('\t')
            if len(cols) not in (2, 4):
                raise ValueError('%s:%d: path<TAB>word[<TAB>start_s<TAB>end_s], got %d columns' % (tsv, no, len(cols)))
            path = cols[0] if os.path.isabs(cols[0]) else os.path.join(here, cols[0])
            start, end = (float(cols[2]), float(cols[3])) if len(cols) == 4 else (None, None)
            out.append((path, cols[1], start, end))
    return out


def clip_length(x):
    """the loader's length rule (dataset.py:52): the index after the last non-zero sample"""
    nz = np.nonzero(x)[0]
    return int(nz[-1]) + 1 if len(nz) else 0


def build_store(entries, out_path=None, sr=8000, maxlen=40000, device=None, rows=256):
    """-> (store, report).  Each file is read once; files of one (rate, channel count, sample kind) are resampled together,
    up to ``rows`` ragged rows per call of ``audio.resample``.  A segment is y[int(start_s sr) : int(end_s sr)] of the
    resampled file (preprocess-fisher.py:145-146); no bounds: the whole file.  A clip is dropped, and counted in
    report['dropped'][reason] with its path, when it is all zero ('silent'), when its length up to the last non-zero
    sample exceeds ``maxlen`` ('too_long'), or when its file cannot be read ('unreadable').  ``store``: word -> float32
    [n_clips, maxlen_word], the clips of a word in entry order; written to ``out_path`` when that is given."""
    entries = list(entries)
    files, groups = {}, collections.OrderedDict()
    report = dict(kept={}, dropped={k: [] for k in DROPPED}, seconds_in=0.0, seconds_out=0.0, files=0)
    for path, _, _, _ in entries:
        if path in files:
            continue
        try:
            data, rate = audio.read_wav(path)
        except (ValueError, OSError) as e:
            files[path] = e
            continue
        files[path] = (data, rate)
        report['files'] += 1
        report['seconds_in'] += data.shape[0] / float(rate)
        groups.setdefault((rate, data.shape[1], data.dtype.str), []).append(path)
    resampled = {}
    for (rate, channels, _), paths in groups.items():
        for i in range(0, len(paths), max(1, int(rows))):
            part = paths[i:i + max(1, int(rows))]
            lens = np.array([files[p][0].shape[0] for p in part], dtype=np.int64)
            batch = np.zeros((len(part), int(lens.max()), channels), dtype=files[part[0]][0].dtype)
            for b, p in enumerate(part):
                batch[b, :lens[b]] = files[p][0]
            y, counts = audio.resample(batch, rate, sr, lens=lens, device=device)
            y = y.cpu().numpy()
            for b, p in enumerate(part):
                resampled[p] = y[b, :counts[b]].copy()
                files[p] = None
    clips = collections.OrderedDict()
    for path, word, start, end in entries:
        if path not in resampled:
            report['dropped']['unreadable'].append(path)
            continue
        y = resampled[path]
        if start is not None:
            y = y[int(start * sr):int(end * sr)]
        n = clip_length(y)
        if n == 0:
            report['dropped']['silent'].append(path)
        elif n > maxlen:
            report['dropped']['too_long'].append(path)
        else:
            clips.setdefault(word, []).append(y[:n])
            report['seconds_out'] += n / float(sr)
    store = {}
    for word, cs in clips.items():
        arr = np.zeros((len(cs), max(len(c) for c in cs)), dtype=np.float32)
        for i, c in enumerate(cs):
            arr[i, :len(c)] = c
        store[word] = arr
        report['kept'][word] = len(cs)
    if out_path is not None:
        save_store(store, out_path)
    return store, report


def save_store(store, path):
    """one uncompressed .npz: 'words' (the keys, in order) and the array of word i under 'w<i>' - a word may hold characters
    a zip member name may not"""
    words = list(store.keys())
    arrays = {'w%d' % i: np.ascontiguousarray(store[w], dtype=np.float32) for i, w in enumerate(words)}
    with open(path, 'wb') as f:
        np.savez(f, words=np.array(words, dtype=np.str_), **arrays)


def load_store(path):
    """the whole store as a dict (an NpzFile would re-read an array at every ``dataset[key]``)"""
    with np.load(path, allow_pickle=False) as z:
        return {str(w): z['w%d' % i] for i, w in enumerate(z['words'])}


def main(argv=None):
    ap = argparse.ArgumentParser(prog='python -m audiogan_amd.ingest', description=__doc__.split('\n\n')[0])
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument('--tree', help='a folder of <word>/*.wav')
    src.add_argument('--manifest', help='a TSV of path, word[, start_s, end_s]')
    ap.add_argument('--out', required=True, help='the .npz to write')
    ap.add_argument('--maxlen', type=int, default=40000)
    ap.add_argument('--device', default=None)
    a = ap.parse_args(argv)
    entries = scan_tree(a.tree) if a.tree else read_manifest(a.manifest)
    store, report = build_store(entries, maxlen=a.maxlen, device=a.device)
    if store:
        save_store(store, a.out)
    print(json.dumps(dict(kept=report['kept'], dropped={k: len(v) for k, v in report['dropped'].items()},
                          dropped_paths=report['dropped'], seconds_in=report['seconds_in'],
                          seconds_out=report['seconds_out']), sort_keys=True))
    return 0 if store else 1


if __name__ == '__main__':
    sys.exit(main())
