"""GPU (-m gpu): mrg_collapse_run called directly (ctypes, device pointers), branch by branch of csrc/collapse.hip, against
plain numpy on the host -- integer work, exact, no tolerance anywhere -- and mrg_ctx_last_collapse says which path
answered: the fast path hands a batch it does not take to the general path silently and both give the same arrays, so
without that record none of these cases could tell a fast path that works from one that overflows on every batch.

Reference: uniques = np.unique of (length << 58 | packed word) -- for one-word reads of at most 29 nt that order IS the
output order --, counts by np.add.at per sample, the length histogram by np.bincount; batches with several words, an N
mask or a 30-nt read (whose word reaches into the length's bits) take a dict keyed by the read instead.

Every output buffer (u_words, u_lens, u_nmask, quant, the length histogram) carries 64 guard elements of a byte pattern
behind `cap`; they must come back untouched.  Inputs may sit at a byte offset of their allocation.

What decides the sizes (restated from fast_prepass and the kernels' constants): a batch is cut into
n_chunks = clamp((n + 8191) / 8192, 1, 1024) chunks of `chunk` = n / n_chunks rounded up to a multiple of 4096 reads, so
chunk is 4096 up to 4096 reads, 8192 up to 2^23 reads and grows only beyond; the first 256 reads of a chunk are its
SAMPLE, from which at most 1024 hot keys are picked; a (rest of key, count) pair counts to 16 383; a reduce table has
2048 slots and gives up above 1536 entries or after a probe of 128 slots."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GUARD = 64            # elements behind every output
PAT = 0xA5            # every guard byte
MASK58 = np.uint64((1 << 58) - 1)
FIELDS = ("path", "reason", "n_chunks", "chunk", "n_hot", "n_pairs", "n_buckets", "n_unique")
GENERAL, FAST, DECLINED, OVERFLOWED = 0, 1, 2, 3                     # last_collapse()["path"]
(NOT_ALLOWED, SEVERAL_WORDS, N_MASK, TOO_MANY_SAMPLES, MISALIGNED,   # last_collapse()["reason"]: 1..8
 TOO_LONG, TOO_MANY_LENGTHS, KEY_TOO_WIDE) = range(1, 9)
K_HOT_KEYS, K_PAIR_MAX_COUNT, K_SAMPLE_READS = 1024, 16383, 256


def planned(n):
    """(n_chunks, chunk) of fast_prepass."""
    n_chunks = max(1, min(1024, (n + 8191) // 8192))
    return n_chunks, ((n + n_chunks - 1) // n_chunks + 4095) & ~4095


class Collapser:
    def __init__(self):
        import torch
        from mirge_amd.engine import Engine
        self.torch = torch
        self.eng = Engine(0)
        self.lib = self.eng._lib
        self.dev = self.eng.device

    def up(self, arr, offset=0):
        """-> (tensor that owns the bytes, device address of arr's first byte = the allocation + offset)."""
        raw = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
        buf = np.full(offset + raw.size + 16, PAT, np.uint8)
        buf[offset:offset + raw.size] = raw
        t = self.torch.from_numpy(buf).to(self.dev)
        assert t.data_ptr() % 256 == 0, "the allocator's own alignment: the offsets below are what they say"
        return t, t.data_ptr() + offset

    def blank(self, n, dtype):
        return self.torch.full(((n + GUARD) * np.dtype(dtype).itemsize,), PAT, dtype=self.torch.uint8, device=self.dev)

    def down(self, t, n, dtype, what):
        a = t.cpu().numpy().view(dtype)
        assert (a[n:].view(np.uint8) == PAT).all(), "%s: written behind its last element" % what
        return a[:n]

    def fast(self, on):
        self.eng.set_option("collapse_fast", 1 if on else 0)

    def info(self):
        return self.eng.last_collapse()

    def run(self, words, lens, sample=None, S=1, nmask=None, cap=None, off_reads=0, off_lens=0, off_sample=0):
        """-> (rc, dict(words [W, U], lens, nmask or None, quant [U, S], hist [256, S], n_unique)); after a refused call
        the dict is None.  The guards are checked either way."""
        words = np.ascontiguousarray(words, dtype=np.uint64)
        words = words.reshape(1, -1) if words.ndim == 1 else words
        W, n = words.shape
        assert n == lens.size
        cap = n if cap is None else cap
        keep = [self.up(words, off_reads), self.up(lens.astype(np.uint8), off_lens)]
        p_nmask = p_sample = None
        if nmask is not None:
            keep.append(self.up(np.ascontiguousarray(nmask, dtype=np.uint64).reshape(W, n)))
            p_nmask = keep[-1][1]
        if sample is not None and S > 1:
            keep.append(self.up(sample.astype(np.uint16), off_sample))
            p_sample = keep[-1][1]
        u_words, u_lens = self.blank(W * cap, np.uint64), self.blank(cap, np.uint8)
        u_nmask = self.blank(W * cap, np.uint64) if nmask is not None else None
        quant, hist = self.blank(cap * S, np.uint32), self.blank(256 * S, np.uint64)
        n_unique = C.c_uint64(0)
        rc = self.lib.mrg_collapse_run(self.eng._h, keep[0][1], W, keep[1][1], p_nmask, p_sample, n, S, 0, cap, u_words.data_ptr(),
                                       u_lens.data_ptr(), None if u_nmask is None else u_nmask.data_ptr(), quant.data_ptr(),
                                       hist.data_ptr(), C.byref(n_unique), self.eng._stream_ptr())
        self.torch.cuda.current_stream(self.dev).synchronize()
        U = int(n_unique.value)
        assert U <= cap
        got = dict(words=self.down(u_words, W * cap, np.uint64, "u_words").reshape(W, cap)[:, :U],
                   lens=self.down(u_lens, cap, np.uint8, "u_lens")[:U],
                   nmask=None if u_nmask is None else self.down(u_nmask, W * cap, np.uint64, "u_nmask").reshape(W, cap)[:, :U],
                   quant=self.down(quant, cap * S, np.uint32, "quant")[:U * S].reshape(U, S),
                   n_unique=U)
        if rc == 0:
            got["hist"] = self.down(hist, 256 * S, np.uint64, "length histogram").reshape(256, S)
        return rc, (got if rc == 0 else None)


@pytest.fixture(scope="module")
def col(native_lib):
    c = Collapser()
    yield c
    c.eng.release_scratch()


# ------------------------------------------------------------------------------------------------ references
def reference(words, lens, sample, S):
    """One-word reads of at most 29 nt -> dict like Collapser.run's."""
    words, lens = np.asarray(words, np.uint64).reshape(-1), np.asarray(lens)
    assert lens.size == 0 or (int(lens.max()) <= 29 and int(words.max()) <= int(MASK58))
    sample = np.zeros(lens.size, np.int64) if sample is None else sample.astype(np.int64)
    key = (lens.astype(np.uint64) << np.uint64(58)) | words
    uniq = np.unique(key)
    quant = np.zeros((uniq.size, S), np.uint32)
    np.add.at(quant, (np.searchsorted(uniq, key), sample), 1)   # (cheaper than return_inverse's argsort at 2^24 reads)
    hist = np.bincount(lens.astype(np.int64) * S + sample, minlength=256 * S).reshape(256, S).astype(np.uint64)
    return dict(words=(uniq & MASK58)[None, :], lens=(uniq >> np.uint64(58)).astype(np.uint8), nmask=None, quant=quant, hist=hist,
                n_unique=uniq.size)


def dict_reference(words, lens, sample, S, nmask=None):
    """Any batch: a dict keyed by the read, ordered by (length, N mask, words), the most significant word first."""
    words = np.asarray(words, np.uint64)
    words = words.reshape(1, -1) if words.ndim == 1 else words
    W, n = words.shape
    nm = np.zeros_like(words) if nmask is None else np.asarray(nmask, np.uint64).reshape(W, n)
    sample = np.zeros(n, np.int64) if sample is None else sample.astype(np.int64)
    want = {}
    cols = [lens.tolist()] + [nm[w].tolist() for w in reversed(range(W))] + [words[w].tolist() for w in reversed(range(W))]
    for key, s in zip(zip(*cols), sample.tolist()):
        want.setdefault(key, [0] * S)[s] += 1
    keys = sorted(want)
    col_of = lambda j: np.array([k[j] for k in keys], np.uint64)
    hist = np.bincount(lens.astype(np.int64) * S + sample, minlength=256 * S).reshape(256, S).astype(np.uint64)
    return dict(words=np.stack([col_of(1 + W + (W - 1 - w)) for w in range(W)]).reshape(W, len(keys)),
                lens=col_of(0).astype(np.uint8),
                nmask=None if nmask is None else np.stack([col_of(1 + (W - 1 - w)) for w in range(W)]).reshape(W, len(keys)),
                quant=np.array([want[k] for k in keys], np.uint32).reshape(len(keys), S), hist=hist, n_unique=len(keys))


def same(got, want, what):
    assert got is not None, what + ": the call was refused"
    assert got["n_unique"] == want["n_unique"], "%s: %d uniques, want %d" % (what, got["n_unique"], want["n_unique"])
    for k in ("lens", "words", "nmask", "quant", "hist"):
        if want[k] is None:
            assert got[k] is None, what
            continue
        bad = np.argwhere(got[k] != want[k])
        assert bad.size == 0, "%s: %s first wrong at %s (got %s, want %s)" % (what, k, bad[0], got[k][tuple(bad[0])], want[k][tuple(bad[0])])


def expect_info(col, what, **fields):
    info = col.info()
    assert sorted(info) == sorted(FIELDS)
    for k, v in fields.items():
        assert info[k] == v, "%s: last_collapse %s = %d, want %d (%s)" % (what, k, info[k], v, info)
    return info


def check_fast(col, words, lens, sample, S, what, want=None, **fields):
    """The batch answers through the fast path with the planned shape and equals the reference."""
    want = reference(words, lens, sample, S) if want is None else want
    rc, got = col.run(words, lens, sample, S)
    assert rc == 0, col.lib.mrg_last_error()
    same(got, want, what)
    n_chunks, chunk = planned(lens.size)
    return expect_info(col, what, path=FAST, reason=0, n_chunks=n_chunks, chunk=chunk, n_unique=want["n_unique"], **fields)


def distinct(rng, k, bits):
    """k distinct values below 2^bits, in random order."""
    v = np.unique(rng.integers(0, 1 << bits, k + k // 4 + 64, dtype=np.uint64))
    assert v.size >= k
    return rng.permutation(v)[:k]


def pool_batch(rng, n, lens_choice, pool_size, S=1, zipf=None):
    pool_len = rng.choice(lens_choice, pool_size).astype(np.uint8)
    pool = rng.integers(0, 1 << 62, pool_size, dtype=np.uint64) & ((np.uint64(1) << (2 * pool_len.astype(np.uint64))) - np.uint64(1))
    pick = rng.integers(0, pool_size, n) if zipf is None else rng.zipf(zipf, n) % pool_size
    return pool[pick], pool_len[pick], rng.integers(0, S, n).astype(np.uint16)


# ------------------------------------------------------------------------------------------------ the record itself
def test_last_collapse_arguments_and_first_state(native_lib):
    from mirge_amd.engine import Engine
    eng = Engine(0)
    assert eng.last_collapse() == dict.fromkeys(FIELDS, 0), "nothing collapsed yet"
    assert eng._lib.mrg_ctx_last_collapse(eng._h, None) < 0 and b"mrg_ctx_last_collapse: null" in eng._lib.mrg_last_error()


# ------------------------------------------------------------------------------------------------ batch sizes and chunk edges
@pytest.mark.parametrize("n,n_chunks,chunk", [(0, 1, 0)] + [(n, 1, 4096) for n in (1, 2, 3, 4, 5, 4095, 4096)] +
                         [(4097, 1, 8192), (8191, 1, 8192), (8192, 1, 8192), (8193, 2, 8192), (24_577, 4, 8192)])
def test_batch_sizes_and_chunk_edges(col, n, n_chunks, chunk):
    """One length, one sample, 50 sequences: the scalar tail of the four-read loads (n = 1..5), a chunk of 4096 and of
    8192 reads, one read short of a chunk, a full one, and chunks whose last holds one read (8193: two chunks, 24 577:
    four)."""
    rng = np.random.default_rng(100 + n)
    words, lens, _ = pool_batch(rng, n, [22], 50)
    if n == 0:
        rc, got = col.run(words, lens)
        assert rc == 0, col.lib.mrg_last_error()
        assert got["n_unique"] == 0 and not got["hist"].any()
        return
    assert planned(n) == (n_chunks, chunk), "the formula as restated here"
    info = check_fast(col, words, lens, None, 1, "n %d" % n)
    assert 1 <= info["n_pairs"] <= n and info["n_buckets"] >= 1


# ------------------------------------------------------------------------------------------------ accepted and declined shapes
N_SHAPE = 3001


def test_shapes_the_fast_path_takes(col):
    """The widest shapes it accepts: 16 distinct lengths; 2 L + sample bits = 58 three ways."""
    rng = np.random.default_rng(21)
    for what, lens_choice, S in (("16 lengths", list(range(10, 26)), 1), ("29 nt", [29], 1), ("28 nt x 4 samples", [28, 19], 4),
                                 ("27 nt x 16 samples", [27, 20], 16)):
        words, lens, sample = pool_batch(rng, N_SHAPE, lens_choice, 700, S)
        assert set(lens.tolist()) == set(lens_choice)
        check_fast(col, words, lens, sample, S, what)


def _declined(col, what, path, reason, words, lens, sample=None, S=1, nmask=None, want=None, **offsets):
    want = reference(words, lens, sample, S) if want is None else want
    rc, got = col.run(words, lens, sample, S, nmask=nmask, **offsets)
    assert rc == 0, col.lib.mrg_last_error()
    same(got, want, what)
    n_chunks, chunk = planned(lens.size) if path == DECLINED else (0, 0)
    expect_info(col, what, path=path, reason=reason, n_chunks=n_chunks, chunk=chunk, n_hot=0, n_pairs=0, n_buckets=0,
                n_unique=want["n_unique"])


def test_shapes_declined_after_the_prepass(col):
    rng = np.random.default_rng(22)
    words, lens, _ = pool_batch(rng, N_SHAPE, list(range(10, 27)), 700)
    assert len(set(lens.tolist())) == 17
    _declined(col, "17 lengths", DECLINED, TOO_MANY_LENGTHS, words, lens)
    words, lens, _ = pool_batch(rng, N_SHAPE, [22], 700)
    words[1234], lens[1234] = np.uint64(0x9A5F1C27B3D4E61), 30             # 60 bits
    _declined(col, "one 30-nt read", DECLINED, TOO_LONG, words, lens, want=dict_reference(words, lens, None, 1))
    words, lens, sample = pool_batch(rng, N_SHAPE, [29, 21], 700, 2)
    _declined(col, "29 nt x 2 samples", DECLINED, KEY_TOO_WIDE, words, lens, sample, 2)


def test_shapes_that_never_enter_the_fast_path(col):
    rng = np.random.default_rng(23)
    words, lens, sample = pool_batch(rng, N_SHAPE, [22, 23], 700, 17)
    _declined(col, "17 samples", GENERAL, TOO_MANY_SAMPLES, words, lens, sample, 17)
    words, lens, sample = pool_batch(rng, N_SHAPE, [22, 23], 700, 2)
    zeros = np.zeros_like(words)
    _declined(col, "an N mask of zeros", GENERAL, N_MASK, words, lens, sample, 2, nmask=zeros,
              want=dict_reference(words, lens, sample, 2, nmask=zeros))
    pick = rng.integers(0, 700, N_SHAPE)
    pool_len = rng.integers(33, 41, 700).astype(np.uint8)
    pool = rng.integers(0, 1 << 62, (2, 700), dtype=np.uint64)
    pool[1] &= (np.uint64(1) << (2 * (pool_len.astype(np.uint64) - np.uint64(32)))) - np.uint64(1)
    pool[1, :350] = pool[1, 350:]                                           # reads that differ in word 0 only
    pool_len[:350] = pool_len[350:]
    two, lens2 = np.ascontiguousarray(pool[:, pick]), pool_len[pick]
    _declined(col, "two words", GENERAL, SEVERAL_WORDS, two, lens2, sample, 2, want=dict_reference(two, lens2, sample, 2))
    _declined(col, "d_lens + 1", GENERAL, MISALIGNED, words, lens, sample, 2, off_lens=1)
    _declined(col, "d_reads + 8", GENERAL, MISALIGNED, words, lens, sample, 2, off_reads=8)
    _declined(col, "d_sample + 2", GENERAL, MISALIGNED, words, lens, sample, 2, off_sample=2)
    _declined(col, "d_lens + 2, one sample", GENERAL, MISALIGNED, words, lens, None, 1, off_lens=2)
    col.fast(False)
    try:
        _declined(col, "collapse_fast = 0", GENERAL, NOT_ALLOWED, words, lens, sample, 2)
    finally:
        col.fast(True)
    check_fast(col, words, lens, sample, 2, "the same batch, aligned and allowed")


# ------------------------------------------------------------------------------------------------ short keys, several samples
def _short_key_batch(rng, S, sparse):
    """(sequence, sample) pairs of 0..12 nt, each 1..3 times, shuffled: every sequence of 0..3 nt in every sample (sparse:
    a random half of those pairs), random ones of 4..12 nt, and per length 2, 4, 5, 6, 7 one sequence in sample S - 1
    only and one in every sample."""
    L, w, s = [], [], []
    for length in range(4):
        for word in range(4 ** length):
            if length == 2 and word in (5, 6):
                continue                        # (the two planted below)
            for smp in range(S):
                if not sparse or rng.random() < 0.5 or (length == 0 and smp == 0):
                    L.append(length), w.append(word), s.append(smp)
    for length in (2, 4, 5, 6, 7):
        L.append(length), w.append(5), s.append(S - 1)
        for smp in range(S):
            L.append(length), w.append(6), s.append(smp)
    for length, k in ((4, 150), (5, 200), (6, 250), (7, 300), (8, 300), (9, 300), (10, 300), (11, 300), (12, 300)):
        word = rng.integers(0, 4 ** length, k)
        ok = (word != 5) & (word != 6)
        L += [length] * int(ok.sum())
        w += word[ok].tolist()
        s += rng.integers(0, S, k)[ok].tolist()
    rep = rng.integers(1, 4, len(L))
    order = rng.permutation(int(rep.sum()))
    return (np.repeat(np.array(w, np.uint64), rep)[order], np.repeat(np.array(L, np.uint8), rep)[order],
            np.repeat(np.array(s, np.uint16), rep)[order])


@pytest.mark.parametrize("sparse", [False, True], ids=["every_pair", "half_the_pairs"])
@pytest.mark.parametrize("S", [2, 3, 16])
def test_short_keys_with_several_samples(col, S, sparse):
    """Reads of at most 7 nt leave fewer than 8 key bits open in their final bucket, so the entries of ONE read (they
    differ in their sample bits only) sit in different bins of reduce_kernel's counting sort: the read is counted once
    only because the kernel looks through the bins in front."""
    words, lens, sample = _short_key_batch(np.random.default_rng(300 + S), S, sparse)
    assert lens.size <= 20_000 and set(range(8)) <= set(lens.tolist())
    want = reference(words, lens, sample, S)
    planted = {(int(l), int(x)): q for l, x, q in zip(want["lens"], want["words"][0], want["quant"]) if x in (5, 6) and l in (2, 4, 5, 6, 7)}
    assert all((planted[(l, 5)][:S - 1] == 0).all() and planted[(l, 5)][S - 1] and planted[(l, 6)].all() for l in (2, 4, 5, 6, 7))
    check_fast(col, words, lens, sample, S, "short keys, %d samples" % S, want=want)


@pytest.mark.parametrize("L,S", [(0, 2), (2, 16), (5, 16), (7, 3)])
def test_heavy_short_key_the_sample_does_not_see(col, L, S):
    """7936 copies of one read of at most 7 nt, spread over the samples, behind 256 singletons: the hot table never sees
    it, so its L1 bucket holds thousands of pairs and is subdivided -- by bits that must stay bases: a final bucket
    boundary between two samples of one read would return the read once per bucket."""
    rng = np.random.default_rng(400 + L)
    n = 8192
    words = np.full(n, 0x1B6D & ((1 << (2 * L)) - 1), np.uint64)
    lens = np.full(n, L, np.uint8)
    words[:K_SAMPLE_READS], lens[:K_SAMPLE_READS] = distinct(rng, K_SAMPLE_READS, 24), 12
    sample = (np.arange(n) % S).astype(np.uint16)
    want = reference(words, lens, sample, S)
    assert want["n_unique"] == 257 and (want["quant"][0] == np.bincount(sample[K_SAMPLE_READS:], minlength=S)).all()
    check_fast(col, words, lens, sample, S, "heavy %d-nt key, %d samples" % (L, S), want=want, n_hot=0, n_pairs=n)


# ------------------------------------------------------------------------------------------------ hot keys
def _sampled_batch(rng, triples):
    """131 072 distinct-by-construction 22-mers in 16 chunks of 8192: a chunk's sample (its first 256 reads) holds k
    sequences three times and (256 - 3 k) / 2 sequences twice, no sequence in two chunks; every read behind the
    sample is a singleton.  k sums to `triples` over the chunks."""
    n, n_chunks, chunk = 131_072, 16, 8192
    assert planned(n) == (n_chunks, chunk)
    fresh = iter(distinct(rng, n, 44).tolist())
    words = np.empty(n, np.uint64)
    twice = 0
    for c in range(n_chunks):
        k = triples // n_chunks + (1 if c < triples % n_chunks else 0)
        m = (K_SAMPLE_READS - 3 * k) // 2
        twice += m
        head = [next(fresh) for _ in range(k)] * 3 + [next(fresh) for _ in range(m)] * 2
        head += [next(fresh) for _ in range(K_SAMPLE_READS - len(head))]
        words[c * chunk:c * chunk + K_SAMPLE_READS] = rng.permutation(np.array(head, np.uint64))
        words[c * chunk + K_SAMPLE_READS:(c + 1) * chunk] = [next(fresh) for _ in range(chunk - K_SAMPLE_READS)]
    return words, np.full(n, 22, np.uint8), twice


def test_hot_key_threshold(col):
    """2048 sample entries of count 2 are more than the hot table holds: the threshold moves above them, no key is hot
    and every read leaves the split as a pair of its own."""
    words, lens, twice = _sampled_batch(np.random.default_rng(51), 0)
    assert twice == 2048 > K_HOT_KEYS
    check_fast(col, words, lens, None, 1, "threshold", n_hot=0, n_pairs=lens.size)


def test_hot_keys_of_mixed_counts(col):
    """500 entries of count 3 in front of 1292 of count 2: exactly the 500 are hot, and each leaves its chunk as one pair
    instead of three."""
    words, lens, twice = _sampled_batch(np.random.default_rng(52), 500)
    assert 500 + twice > K_HOT_KEYS
    check_fast(col, words, lens, None, 1, "mixed counts", n_hot=500, n_pairs=lens.size - 2 * 500)


def test_cold_heavy_key(col):
    """A sequence that is 97 % of the batch but absent from the sample is not hot: 7936 pairs of count 1, summed by the
    reduce table."""
    rng = np.random.default_rng(53)
    n = 8192
    v = distinct(rng, K_SAMPLE_READS + 1, 44)
    words = np.full(n, v[-1], np.uint64)
    words[:K_SAMPLE_READS] = v[:-1]
    lens = np.full(n, 22, np.uint8)
    want = reference(words, lens, None, 1)
    assert want["n_unique"] == 257 and int(want["quant"].max()) == n - K_SAMPLE_READS == 7936
    check_fast(col, words, lens, None, 1, "cold heavy key", want=want, n_hot=0, n_pairs=n)


# ------------------------------------------------------------------------------------------------ reduce table
@pytest.mark.parametrize("D", [1000, 1536, 1537, 2000])
def test_reduce_table_load(col, D):
    """D distinct 22-mers that share their 8 most significant bases fall into ONE final bucket.  1000 entries load the
    2048 slots to 0.49 (a probe of 128 occupied slots in a row cannot happen): the fast path answers; 2000 are above the
    1536-entry bound: the general path answers; at the bound itself the probe lengths decide, and either is right."""
    rng = np.random.default_rng(600 + D)
    words = (np.uint64(0x9C3A) << np.uint64(28)) | distinct(rng, D, 28)
    lens = np.full(D, 22, np.uint8)
    want = reference(words, lens, None, 1)
    assert want["n_unique"] == D
    rc, got = col.run(words, lens)
    assert rc == 0, col.lib.mrg_last_error()
    same(got, want, "D %d" % D)
    info = expect_info(col, "D %d" % D, reason=0, n_chunks=1, chunk=4096, n_hot=0, n_pairs=D, n_buckets=1, n_unique=D)
    assert info["path"] in {1000: (FAST,), 2000: (OVERFLOWED,)}.get(D, (FAST, OVERFLOWED)), info


# ------------------------------------------------------------------------------------------------ beyond 2^23 reads
def test_chunks_past_the_end_of_the_batch(col):
    """2^23 + 1 reads (Zipf over 100 000 sequences of 20..23 nt): the first size at which a chunk is not 8192 reads --
    12 288 -- and at which 1024 chunks cover more than the batch: chunk 682 is cut short and chunks 683..1023 hold nothing."""
    n = (1 << 23) + 1
    assert planned(n) == (1024, 12_288) and -(-n // 12_288) == 683
    words, lens, _ = pool_batch(np.random.default_rng(71), n, [20, 21, 22, 23], 100_000, zipf=1.2)
    info = check_fast(col, words, lens, None, 1, "2^23 + 1 reads")
    assert info["n_hot"] >= 1 and info["n_pairs"] < n


def test_a_hot_count_leaves_its_chunk_in_pieces(col):
    """2^24 reads in chunks of 16 384: reads 0..99 999 and half of the rest are ONE sequence, so chunks 0..5 are that
    sequence 16 384 times -- one more than a pair's 14-bit count holds: split_kernel's piece loop writes two pairs for it.
    (n_hot >= 1 and fewer than n / 2 pairs: the hot table did absorb the sequence; its exact count: no piece was lost.)"""
    n = 1 << 24
    assert planned(n) == (1024, 16_384) and 16_384 > K_PAIR_MAX_COUNT and 99_999 // 16_384 == 6
    rng = np.random.default_rng(72)
    words, lens, _ = pool_batch(rng, n, [22], 50_000)
    hot = np.uint64(0x2B3C4D5E6F7)
    is_hot = rng.random(n) < 0.5
    is_hot[:100_000] = True
    words[is_hot] = hot
    want = reference(words, lens, None, 1)
    at = int(np.searchsorted(want["words"][0], hot))
    assert want["words"][0, at] == hot and want["quant"][at, 0] >= int(is_hot.sum()) > n // 2
    info = check_fast(col, words, lens, None, 1, "2^24 reads", want=want)
    assert info["n_hot"] >= 1 and info["n_pairs"] < n // 2, info


# ------------------------------------------------------------------------------------------------ cap and sample ids
@pytest.mark.parametrize("fast", [True, False], ids=["fast_path", "general_path"])
def test_cap_is_checked_and_exactly_enough(col, fast):
    from mirge_amd._native import MRG_ERR_ARG
    rng = np.random.default_rng(81)
    words, lens, sample = pool_batch(rng, 3000, [21, 22], 500, 3)
    want = reference(words, lens, sample, 3)
    U = want["n_unique"]
    assert 400 < U <= 500
    col.fast(fast)
    try:
        rc, got = col.run(words, lens, sample, 3, cap=U)
        assert rc == 0, col.lib.mrg_last_error()
        same(got, want, "cap = U")
        before = expect_info(col, "cap = U", path=FAST if fast else GENERAL, reason=0 if fast else NOT_ALLOWED, n_unique=U)
        rc, got = col.run(words, lens, sample, 3, cap=U - 1)
        assert rc == MRG_ERR_ARG and got is None
        assert b"cap %d" % (U - 1) in col.lib.mrg_last_error()
        assert col.info() == before, "a refused call leaves the record alone"
    finally:
        col.fast(True)


def test_sample_id_out_of_range_on_the_general_path(col):
    from mirge_amd._native import MRG_ERR_ARG
    rng = np.random.default_rng(82)
    words, lens, sample = pool_batch(rng, 3000, [22], 500, 2)
    sample[2999] = 2
    col.fast(False)
    try:
        rc, got = col.run(words, lens, sample, 2)
        assert rc == MRG_ERR_ARG and got is None and b"sample id" in col.lib.mrg_last_error()
    finally:
        col.fast(True)
