"""The reference's minibatch-generator interface (dataset.py:1-118) with a pluggable backing
store.  Same function names, arguments and return tuples:

  dataloader(batch_size, args, maxlen=None, frame_size=None)
      conditional   -> (dataset, maxlen, gen_train, gen_val, keys_train, keys_val)      (:110)
          next(gen) -> [epoch, batch, samples (B, maxlen^frame) f64, lengths (B,), keys,
                        cseq (B, maxchar) i32, clen (B,)]                               (:91)
      unconditional -> (None, gen_train, gen_val)                                       (:41)
          next(gen) -> [epoch, batch, (B, amplitudes)] + [None] * 6                     (:25)
  pick_words(batch_size, maxlen, dataset, keys, maxcharlen, args, frame_size=None, skip_samples=False)
      -> [keys, cseq, clen, samples, lengths] as numpy arrays                          (:76-77)

``args.dataset`` may be (a) a path to an HDF5 file in the reference's layout -- word-keyed
datasets of shape (n, maxlen_word), zero padded (needs h5py, which this image lacks), (a') a path ending in ``.npz``: the
same layout as written by ``audiogan_amd.ingest`` from WAV files (``ingest.load_store``, no h5py), or (b) an
in-memory mapping with the same layout, e.g. ``SyntheticWordDataset`` / ``{'data': array}``,
which is what bench/tests use (SURVEY.md 8(d) synthetic clips).  Randomness comes from the
global numpy RNG exactly like the reference (RNG.choice / RNG.permutation).

Beyond the reference, opt-in: ``args.device_store = 'cuda'`` keeps every clip on that device (``DeviceWordStore``); the
conditional loader then draws clip ids with the same RNG calls and yields a ``ClipBatch`` where the host loader yields the
float64 array (``device_dataloader``, at the end of this file).
"""
import numpy as NP
import numpy.random as RNG


def div_roundup(x, d):
    """utiltf.py:102-103"""
    return (x + d - 1) // d


def roundup(x, d):
    """utiltf.py:105-106"""
    return div_roundup(x, d) * d


class SyntheticWordDataset(dict):
    """word -> float32 array (n_utterances, maxlen_word), zero padded at the end, the on-disk layout
    written by preprocess-fisher.py:240-250.  kind 'noise' = U(-1,1), 'sine' = 100..1000 Hz tones."""

    def __init__(self, words, n_per_word=4, min_len=2000, max_len=8192, kind='noise', seed=0):
        super().__init__()
        rs = NP.random.RandomState(seed)
        for w in words:
            arr = NP.zeros((n_per_word, max_len), dtype=NP.float32)
            for i in range(n_per_word):
                n = int(rs.randint(min_len, max_len + 1))
                if kind == 'sine':
                    f = rs.uniform(100, 1000)
                    arr[i, :n] = NP.sin(2 * NP.pi * f * NP.arange(n) / 8000.0)
                else:
                    arr[i, :n] = rs.uniform(-1, 1, size=n)
                arr[i, n - 1] = arr[i, n - 1] if arr[i, n - 1] != 0 else 0.5   # length = last non-zero
            self[w] = arr


def _open(spec):
    if isinstance(spec, str):
        if spec.endswith('.npz'):          # a word store written by audiogan_amd.ingest: loaded whole, no h5py
            from . import ingest
            return ingest.load_store(spec)
        try:
            import h5py
        except ImportError as e:
            raise ImportError('args.dataset is a path but h5py is not installed; pass an in-memory '
                              'mapping (e.g. audiogan_amd.dataset.SyntheticWordDataset)') from e
        return h5py.File(spec, 'r')
    return spec


def _unconditional_dataloader(batch_size, data, lower, upper, args):
    """dataset.py:6-25"""
    epoch, batch = 1, 0
    idx = RNG.permutation(range(lower, upper))
    cur = 0
    while True:
        indices = []
        for _ in range(batch_size):
            if cur == len(idx):
                cur = 0
                idx = RNG.permutation(list(set(range(lower, upper)) - set(indices)))
                epoch += 1
                batch = 0
            indices.append(idx[cur])
            cur += 1
        sample = data[sorted(indices)]
        yield [epoch, batch, NP.array(sample)[:, :args.amplitudes]] + [None] * 6
        batch += 1


def unconditional_dataloader(batch_size, args):
    """dataset.py:27-41"""
    dataset = _open(args.dataset)
    data = dataset['data']
    nsamples = data.shape[0]
    if getattr(args, 'subset', None):
        keep = RNG.permutation(range(nsamples))[:args.subset]
        data = data[sorted(keep)]
        nsamples = args.subset
    n_train = nsamples // 10 * 9
    return (None, _unconditional_dataloader(batch_size, data, 0, n_train, args),
            _unconditional_dataloader(batch_size, data, n_train, nsamples, args))


def word_to_seq(word, maxcharlen):
    """dataset.py:43-46"""
    seq = NP.zeros(maxcharlen, dtype=NP.int32)
    seq[:len(word)] = [ord(ch) for ch in word]
    return seq


def _pick_sample_from_word(key, maxlen, dataset, frame_size=None, skip_samples=False):
    """dataset.py:48-61: random utterance of `key`; length = index after the last non-zero sample,
    rounded up to a whole number of frames; (None, None) when it does not fit in maxlen."""
    sample_idx = RNG.choice(dataset[key].shape[0])
    out = NP.zeros(maxlen)
    length = 0
    if not skip_samples:
        src = NP.asarray(dataset[key][sample_idx])
        nz = NP.nonzero(src)[0]
        n = int(nz[-1]) + 1 if len(nz) else 0
        if n > maxlen:
            return None, None
        length = n if frame_size is None else roundup(n, frame_size)
        out[:n] = src[:n]
    return out, length


def pick_word(maxlen, dataset, keys, maxcharlen, args, frame_size=None, skip_samples=False):
    """dataset.py:63-74: redraw until a clip fits and is not silent; peak-normalise (:68-71)"""
    while True:
        key = RNG.choice(keys)
        out, length = _pick_sample_from_word(key, maxlen, dataset, frame_size, skip_samples)
        if out is None:
            continue
        if not skip_samples:
            peak = NP.abs(out).max()
            if peak == 0:
                continue
            out /= peak
        break
    return key, word_to_seq(key, maxcharlen), len(key), out, length


def pick_words(batch_size, maxlen, dataset, keys, maxcharlen, args, frame_size=None, skip_samples=False):
    """dataset.py:76-77"""
    picks = [pick_word(maxlen, dataset, keys, maxcharlen, args, frame_size, skip_samples)
             for _ in range(batch_size)]
    return [NP.array(col) for col in zip(*picks)]


def _conditional_dataloader(batch_size, dataset, maxlen, keys, args, frame_size=None):
    """dataset.py:79-91"""
    epoch, batch = 0, 0
    maxcharlen = max(len(k) for k in keys)
    if frame_size is not None:
        maxlen = roundup(maxlen, frame_size)
    while True:
        batch += 1
        picked, cseq, clen, samples, lengths = pick_words(batch_size, maxlen, dataset, keys, maxcharlen,
                                                          args, frame_size)
        yield [epoch, batch, samples, lengths, picked, cseq, clen]


def _valid_keys(keys, args):
    """dataset.py:93-96"""
    keys = [k for k in keys if not (k[-1] == '-' or k[0] == '(')]
    return [k for k in keys if len(k) >= args.minwordlen]


def conditional_dataloader(batch_size, args, maxlen=None, frame_size=None):
    """dataset.py:98-110"""
    dataset = _open(args.dataset)
    keys = _valid_keys(list(dataset.keys()), args)
    keys = [str(k) for k in RNG.permutation(keys)]
    n_train = len(keys) // 10 * 9
    maxlen = maxlen or max(dataset[k].shape[1] for k in keys)
    train_keys, val_keys = keys[:n_train], keys[n_train:]
    return (dataset, maxlen,
            _conditional_dataloader(batch_size, dataset, maxlen, train_keys, args, frame_size),
            _conditional_dataloader(batch_size, dataset, maxlen, val_keys, args, frame_size),
            train_keys, val_keys)


def dataloader(batch_size, args, maxlen=None, frame_size=None):
    """dataset.py:112-118; ``args.device_store`` (a device, e.g. 'cuda'; beyond the reference): the conditional loader over a
    ``DeviceWordStore`` on that device (``device_dataloader``)"""
    if not args.conditional:
        return unconditional_dataloader(batch_size, args)
    if getattr(args, 'device_store', None) is not None:
        return device_dataloader(batch_size, args, args.device_store, maxlen=maxlen, frame_size=frame_size)
    return conditional_dataloader(batch_size, args, maxlen=maxlen, frame_size=frame_size)


# --------------------------------------------------------------------------------------
# The device-resident word store (beyond the reference): every clip stays on the device, packed; the host only draws WHICH
# clips make a minibatch - with the reference's RNG calls, in its order - and one launch (kernels.clip_gather) writes the
# peak-normalised, zero-padded float32 rows and their lengths where the step reads them.  What pick_word repeats on the same
# clips at every draw (the scan for the last non-zero sample, the peak, a float64 row of maxlen) is done once, by
# kernels.clip_facts, when the store is built.
#   bank   float32  clip c is bank[start[c] : start[c] + cap[c]], clips in word order, then row order
#   start  int64    a multiple of 4 floats each (16-byte loads), the gaps and the end of the bank zero
#   cap    int32    the word's row width
# --------------------------------------------------------------------------------------
class _Rows(object):
    """what ``store[key]`` answers: the shape the loader functions read (``dataset[key].shape``)"""

    def __init__(self, shape):
        self.shape = shape


class DeviceWordStore(object):
    PIECE = 1 << 22          # floats of the pinned buffer the bank is uploaded through

    def __init__(self, mapping, device, piece=None):
        """``mapping``: word -> float32 [n_clips, maxlen_word], zero padded (``ingest.load_store``, ``SyntheticWordDataset``,
        an open HDF5 file).  Raises ValueError for a word without clips and for a clip that holds a NaN or an infinity."""
        import torch
        from . import kernels as K
        self.dev = torch.device(device)
        self._words, self._first, self._shape = [], {}, {}
        caps, owner = [], []
        for w in mapping.keys():
            shape = tuple(int(s) for s in mapping[w].shape)
            if len(shape) != 2 or shape[0] < 1 or shape[1] >= 2 ** 31:
                raise ValueError('DeviceWordStore: word %r has shape %r; [n_clips >= 1, maxlen_word] is needed' % (w, shape))
            w = str(w)
            self._words.append(w)
            self._first[w], self._shape[w] = len(caps), shape
            caps += [shape[1]] * shape[0]
            owner += [w] * shape[0]
        self.n_clips = len(caps)
        cap = NP.asarray(caps, dtype=NP.int64)
        slot = (cap + 3) // 4 * 4          # every start a multiple of 4 floats
        start = NP.concatenate([[0], NP.cumsum(slot)[:-1]]).astype(NP.int64) if self.n_clips else NP.zeros(0, NP.int64)
        total = int(slot.sum())
        self.start_host, self.cap_host = start, cap.astype(NP.int32)
        self.bank = torch.empty(total, dtype=torch.float32, device=self.dev)
        self._upload(mapping, int(piece or self.PIECE))
        self.start = torch.from_numpy(start).to(self.dev)
        self.cap = torch.from_numpy(self.cap_host).to(self.dev)
        n, peak = K.clip_facts(self.bank, self.start, self.cap)
        self.n_dev, self.peak = n, peak
        self.n = n.cpu().numpy()          # (the one read)
        bad = NP.nonzero(~NP.isfinite(peak.cpu().numpy()))[0]
        if len(bad):
            c = int(bad[0])
            raise ValueError('DeviceWordStore: clip %d of word %r holds a NaN or an infinity' % (c - self._first[owner[c]], owner[c]))
        self.silent = self.n == 0

    @classmethod
    def from_npz(cls, path, device, piece=None):
        """the store of a file written by ``audiogan_amd.ingest``"""
        from . import ingest
        return cls(ingest.load_store(path), device, piece=piece)

    def _upload(self, mapping, piece):
        """the bank through one buffer of ``piece`` floats - pinned when the store is on a GPU - filled by numpy's own copy
        (train.Feeder.stage says why) and sent piece by piece; gaps between clips and the end of the bank are zero"""
        import torch
        piece = max(4, piece // 4 * 4)
        total = self.bank.numel()
        pin = torch.zeros(min(piece, max(total, 1)), dtype=torch.float32, pin_memory=self.dev.type == 'cuda')
        buf = pin.numpy()
        base = 0

        def flush():
            k = min(len(buf), total - base)
            self.bank[base:base + k].copy_(pin[:k], non_blocking=True)
            if self.dev.type == 'cuda':
                torch.cuda.current_stream().synchronize()          # (the buffer is refilled next)
            buf[...] = 0
            return base + k

        c = 0
        for w in self._words:
            arr = mapping[w]
            for i in range(self._shape[w][0]):
                row = NP.asarray(arr[i], dtype=NP.float32)
                at, done = int(self.start_host[c]), 0
                while done < len(row):
                    while at + done >= base + len(buf):
                        base = flush()
                    k = min(len(row) - done, base + len(buf) - (at + done))
                    buf[at + done - base:at + done - base + k] = row[done:done + k]
                    done += k
                c += 1
        while base < total:
            base = flush()

    # ---- what the loader functions read ----
    def keys(self):
        return list(self._words)

    def __getitem__(self, key):
        return _Rows(self._shape[str(key)])

    def __contains__(self, key):
        return str(key) in self._shape

    def __len__(self):
        return len(self._words)

    def pick_words(self, batch_size, maxlen, keys, maxcharlen, frame_size=None, skip_samples=False):
        """``pick_words`` over the store -> [keys, cseq, clen, ClipBatch, lengths]: the calls to the global numpy RNG of the
        host function in its order (RNG.choice(keys), RNG.choice(n_clips); both again when the clip is longer than ``maxlen``
        or silent), so keys, character arrays, lengths and the RNG state afterwards are the host function's"""
        picked, ids, lengths = [], [], []
        for _ in range(batch_size):
            while True:
                key = RNG.choice(keys)
                c = self._first[str(key)] + RNG.choice(self._shape[str(key)][0])
                if skip_samples:
                    n = 0
                    break
                n = int(self.n[c])
                if n > maxlen or self.silent[c]:
                    continue
                break
            picked.append(key)
            ids.append(c)
            lengths.append(n if frame_size is None else roundup(n, frame_size))
        cseq = NP.array([word_to_seq(k, maxcharlen) for k in picked])
        clen = NP.array([len(k) for k in picked])
        batch = ClipBatch(self, ids, maxlen, frame_size, empty=skip_samples)
        return [NP.array(picked), cseq, clen, batch, NP.array(lengths)]


class ClipBatch(object):
    """the clips of one minibatch as ids into a ``DeviceWordStore``: ``gather`` writes the rows on the device; as an array
    (``shape``, ``numpy.asarray``, indexing) it is the float32 [B, L_out] minibatch, read back once"""

    def __init__(self, store, ids, L_out, frame=None, empty=False):
        ids = NP.ascontiguousarray(ids, dtype=NP.int64).reshape(-1)
        if len(ids) and (ids.min() < 0 or ids.max() >= store.n_clips):
            raise ValueError('ClipBatch: clip ids %d .. %d; the store holds %d clips' % (ids.min(), ids.max(), store.n_clips))
        self.store, self.ids, self.L_out, self.frame = store, ids, int(L_out), (int(frame) if frame else 0)
        self.empty = bool(empty)          # pick_words(skip_samples=True): rows of zeros, lengths 0, as the host function's
        self.shape = (len(ids), self.L_out)
        self.dtype = NP.dtype(NP.float32)
        self._ids_dev = self._host = None

    def __len__(self):
        return len(self.ids)

    def gather(self, out=None, len_out=None, ids=None):
        """one ``kernels.clip_gather`` on the current stream -> (out, len_out): into the given tensors (``out`` [B, W] float32
        of any width W >= 1 - a narrower one crops, a wider one is zero-filled - and ``len_out`` int64 [B]) or into fresh
        ones of width L_out.  ``ids``: the batch's ids already on the device (train.Feeder's staged copy)"""
        import torch
        from . import kernels as K
        st = self.store
        if out is None:
            out = torch.empty(self.shape, dtype=torch.float32, device=st.dev)
        if len_out is None:
            len_out = torch.empty(len(self.ids), dtype=torch.int64, device=st.dev)
        if self.empty:
            return out.zero_(), len_out.zero_()
        if ids is None:
            if self._ids_dev is None:
                # (through pinned memory, without waiting: a pageable upload would hold the host until the stream has
                # drained, and an eager loop lives on running ahead of the device)
                pin = torch.empty(len(self.ids), dtype=torch.int64, pin_memory=st.dev.type == 'cuda')
                pin.numpy()[...] = self.ids
                self._ids_dev = pin.to(st.dev, non_blocking=True)
            ids = self._ids_dev
        return K.clip_gather(st.bank, st.start, st.n_dev, st.peak, ids, out, len_out, self.frame)

    def __array__(self, dtype=None, copy=None):
        if self._host is None:
            self._host = self.gather()[0].cpu().numpy()          # (one gather, one read)
        return self._host if dtype is None else self._host.astype(dtype, copy=False)

    def __getitem__(self, idx):
        return self.__array__()[idx]


def _device_conditional_dataloader(batch_size, store, maxlen, keys, frame_size=None):
    """``_conditional_dataloader`` over the store: ``samples`` is a ``ClipBatch``"""
    epoch, batch = 0, 0
    maxcharlen = max(len(k) for k in keys)
    if frame_size is not None:
        maxlen = roundup(maxlen, frame_size)
    while True:
        batch += 1
        picked, cseq, clen, samples, lengths = store.pick_words(batch_size, maxlen, keys, maxcharlen, frame_size)
        yield [epoch, batch, samples, lengths, picked, cseq, clen]


def device_dataloader(batch_size, args, device, maxlen=None, frame_size=None):
    """``conditional_dataloader`` with a ``DeviceWordStore`` on ``device`` in the dataset's place (``args.dataset`` may be
    one already): the same key filter, permutation and 90/10 split, the same 6-tuple; the two generators yield a
    ``ClipBatch`` where the host ones yield the float64 array"""
    dataset = _open(args.dataset)
    store = dataset if isinstance(dataset, DeviceWordStore) else DeviceWordStore(dataset, device)
    keys = _valid_keys(list(store.keys()), args)
    keys = [str(k) for k in RNG.permutation(keys)]
    n_train = len(keys) // 10 * 9
    maxlen = maxlen or max(store[k].shape[1] for k in keys)
    train_keys, val_keys = keys[:n_train], keys[n_train:]
    return (store, maxlen,
            _device_conditional_dataloader(batch_size, store, maxlen, train_keys, frame_size),
            _device_conditional_dataloader(batch_size, store, maxlen, val_keys, frame_size),
            train_keys, val_keys)
