"""Columnar host API over the C-ABI: one Engine per GPU.

This is the scale path (10^7..10^8 reads): packed reads, counts and
assignments live in HBM as flat arrays instead of the reference's dict of dicts
(`seqDic`, MAIN:318-321; infeasible at 10^8 entries).  `mirge_amd.annotate`
materialises the reference's dict shapes from these arrays for small inputs.

torch is used only for device memory, streams and (in mirge_amd.dist)
torch.distributed; every kernel is launched through libmirge_amd.so.
"""
import contextlib
import ctypes as C

import numpy as np

from . import _native
from ._native import PassCfg, PassStats, check

V_MODE_SEED = 1024  # "-v": the seed region is the whole read
DEFAULT_WSTOP = 8    # the context's default "wstop" option (mrg_ctx_set_option)

# The nine (ten) bowtie command lines of runAnnotationPipeline.py:577-599 / :688:
# (library key, min_len, max_len, seed_len, max_mm_seed, max_mm_total, trim5, trim3, poly_t)
MIRGE_PASS_TABLE = [
    ("mirna", 0, 25, 28, 0, 2, 0, 0, 0),                    # len < 26 ; -n 0
    ("hairpin", 26, 255, 28, 1, 2, 0, 0, 0),                # len > 25 ; -n 1
    ("mature_trna", 0, 255, V_MODE_SEED, 1, 1, 0, 0, 0),    # -v 1 -a --best --strata
    ("pre_trna", 0, 255, V_MODE_SEED, 0, 0, 0, 0, 1),       # poly-T rule ; -v 0 -a --best --strata
    ("snorna", 0, 255, 28, 1, 2, 0, 0, 0),                  # -n 1
    ("rrna", 0, 255, 28, 1, 2, 0, 0, 0),                    # -n 1
    ("ncrna_others", 0, 255, 28, 1, 2, 0, 0, 0),            # -n 1
    ("mrna", 0, 255, 28, 0, 2, 0, 0, 0),                    # -n 0
    ("mirna", 0, 255, V_MODE_SEED, 2, 2, 1, 2, 0),          # -5 1 -3 2 -v 2 --best
    ("spike-in", 0, 255, 28, 0, 2, 0, 0, 0),                # -n 0 (only with -spikeIn)
]
# libraries a pass searches WITHOUT seed mismatch: a large one of them gets an exact-match dictionary too
EXACT_LIBS = frozenset(row[0] for row in MIRGE_PASS_TABLE if row[4] == 0)
DICT_SMALL_BASES = 1 << 22   # csrc/dict_index.hpp: kDictSmallBases / kDictMaxBases
DICT_MAX_BASES = 1 << 30
STRATUM_BEST, STRATUM_ALL = 0, 1  # mrg_list_valid_fill: MRG_STRATUM_BEST / MRG_STRATUM_ALL
CANON_PASS = 0   # annot slot 1 "exact miRNA"
ISOMIR_PASS = 8  # annot slot 9 "isomiR miRNA"


def _torch():
    import torch
    return torch


class _Marks:
    """Device events in a row, for a call that reports the milliseconds between them.  mark() records the next one: on the
    current stream of `device`, or, without a device, where Event.record() itself records (the current stream of the
    current device).  ms(a, b) waits for the last mark.  With timings None, mark() does nothing."""

    def __init__(self, timings, device=None):
        self.on, self.device, self.ev = timings is not None, device, []

    def mark(self):
        if self.on:
            torch = _torch()
            e = torch.cuda.Event(enable_timing=True)
            if self.device is None:
                e.record()
            else:
                e.record(torch.cuda.current_stream(self.device))
            self.ev.append(e)

    def ms(self, a, b):
        self.ev[-1].synchronize()
        return self.ev[a].elapsed_time(self.ev[b])


@contextlib.contextmanager
def _timed(timings, key):
    """timings[key] = the device milliseconds of the block, between two events of Event.record(); nothing when timings is
    None, and no entry when the block raises."""
    m = _Marks(timings)
    m.mark()
    yield
    m.mark()
    if timings is not None:
        timings[key] = m.ms(0, 1)


class ReadSet:
    """Packed reads resident in HBM."""

    def __init__(self, words, lens, nmask=None, quant=None, device="cuda:0"):
        torch = _torch()
        words = np.ascontiguousarray(words, dtype=np.uint64)
        self.W, self.n = words.shape
        self.device = torch.device(device)
        self.words = torch.from_numpy(words.view(np.int64)).to(self.device)
        lens = np.ascontiguousarray(lens, dtype=np.uint8)
        self.min_len = int(lens.min()) if lens.size else 0
        self.max_len = int(lens.max()) if lens.size else 255
        self.lens = torch.from_numpy(lens).to(self.device)
        self.nmask = None
        if nmask is not None:
            nm = np.ascontiguousarray(nmask, dtype=np.uint64)
            self.nmask = torch.from_numpy(nm.view(np.int64)).to(self.device)
        self.quant = None
        if quant is not None:
            q = np.ascontiguousarray(quant, dtype=np.uint32)
            if q.ndim == 1:
                q = q[:, None]
            self.quant = torch.from_numpy(q.view(np.int32)).to(self.device)

    @classmethod
    def from_device(cls, words, lens, nmask=None, quant=None, min_len=0, max_len=255):
        """Wrap tensors that already live in HBM (words int64 [W, n], lens uint8 [n], nmask like
        words or None, quant int32 [n, S] or None): nothing is copied.  min_len / max_len is the
        caller's knowledge of the batch's length range (0 / 255 = unknown)."""
        self = cls.__new__(cls)
        self.W, self.n = int(words.shape[0]), int(words.shape[1])
        self.device = words.device
        self.words, self.lens, self.nmask, self.quant = words, lens, nmask, quant
        self.min_len, self.max_len = int(min_len), int(max_len)
        return self

    @property
    def n_samples(self):
        return 0 if self.quant is None else int(self.quant.shape[1])


class CascadeResult:
    def __init__(self, pass_id, ref_id, pos, mm, pass_counts, engine, n_pass, packed=None):
        self.pass_id, self.ref_id, self.pos, self.mm = pass_id, ref_id, pos, mm
        self.packed = packed            # device int32 [n] (Engine.cascade_packed): then the four arrays are None
        self.pass_counts = pass_counts  # device int64 [2*n_pass]: processed, aligned
        self._engine = engine
        self.n_pass = n_pass
        self._stats = None
        self._run_id = engine._run_id() if engine is not None and hasattr(engine, "_run_id") else None

    @property
    def stats(self):
        """Synchronises; list of dicts per pass."""
        if self._stats is None:
            if self._run_id is not None and self._engine._run_id() != self._run_id:
                raise RuntimeError("the context has run another cascade since: read `stats` of a result before "
                                   "launching the next one (the counters and event times live in the context)")
            self._stats = self._engine._read_stats(self.n_pass)
        return self._stats

    def to_host(self):
        if self.packed is not None:   # (entries and offsets saturate: unpack_assignments)
            return unpack_assignments(self.packed.cpu().numpy())
        return (self.pass_id.cpu().numpy(), self.ref_id.cpu().numpy(), self.pos.cpu().numpy(),
                self.mm.cpu().numpy())


class Engine:
    def __init__(self, device=0):
        self._lib = _native.load()
        h = C.c_void_p()
        check(self._lib.mrg_ctx_create(int(device), C.byref(h)))
        self._h = h
        self.device_index = int(device)
        self.device = "cuda:%d" % int(device)
        self.libs = {}      # key -> lib id
        self.indexes = {}   # key -> FmIndex (kept alive; names for reports)
        self._ws = None
        n_cu = C.c_int32()
        hbm = C.c_uint64()
        arch = C.create_string_buffer(64)
        check(self._lib.mrg_ctx_device_info(self._h, C.byref(n_cu), C.byref(hbm), arch, 64))
        self.n_cu, self.hbm_bytes, self.arch = n_cu.value, hbm.value, arch.value.decode()
        # development aid: MIRGE_AMD_OPTS="key=value,key=value" sets context options on every new engine (A/B runs
        # of the whole test suite under another kernel variant)
        import os
        for kv in filter(None, os.environ.get("MIRGE_AMD_OPTS", "").split(",")):
            k, v = kv.split("=")
            self.set_option(k.strip(), int(v))

    def close(self):
        if getattr(self, "_h", None):
            self._lib.mrg_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_option(self, key, value):
        check(self._lib.mrg_ctx_set_option(self._h, key.encode(), int(value)))

    def release_scratch(self):
        """Free the context's scratch arena (the collapse keeps 40 B per raw read otherwise)."""
        check(self._lib.mrg_ctx_release_scratch(self._h))

    def add_library(self, key, index, exact_dict=None):
        """Make a library resident.  exact_dict: give a LARGE library (> 4 Mbp) an exact-match dictionary
        too (16 B x 2..4 slots per base of HBM) -- by default the libraries the reference cascade searches
        without a seed mismatch (mRNA `-n 0`, runAnnotationPipeline.py:584/598; spike-in, :586): one 16-byte
        gather per read instead of a jump-table line and a suffix-array row line.  Small libraries always
        get theirs."""
        if exact_dict is None:
            exact_dict = key in EXACT_LIBS
        self.set_option("dict_max_bases", DICT_MAX_BASES if exact_dict else DICT_SMALL_BASES)
        lid = C.c_int32(-1)
        check(self._lib.mrg_ctx_add_library(self._h, index._h, C.byref(lid)))
        self.libs[key] = lid.value
        self.indexes[key] = index
        return lid.value

    def library_dict_stats(self, key):
        """(positions stored in the library's exact-match dictionary, HOME SLOTS whose chain overflowed -- every further
        position of such a home is left to the FM index: a count of homes, not of positions) -- mrg_ctx_library_stats."""
        out = (C.c_uint64 * 4)()
        check(self._lib.mrg_ctx_library_stats(self._h, self.libs[key], out))
        return int(out[0]), int(out[1])

    def check_tables(self, key):
        """Words in which a resident library's jump tables / row context / wide rows / seed buckets differ from the host
        functions' (None = the library has no such table) -- mrg_ctx_library_check_tables: 0 everywhere is the bar."""
        out = (C.c_uint64 * 4)()
        check(self._lib.mrg_ctx_library_check_tables(self._h, self.libs[key], self.indexes[key]._h, out))
        names = ("jump_tables", "row_context", "wide_rows", "seed_buckets")
        return {n: (None if int(v) == 2 ** 64 - 1 else int(v)) for n, v in zip(names, out)}

    # ------------------------------------------------------------------
    def mirge_passes(self, spike_in=False):
        """PassCfg array for the reference's cascade (runAnnotationPipeline.py:574-599)."""
        rows = MIRGE_PASS_TABLE[:10 if spike_in else 9]
        return self.make_passes([dict(lib=k, min_len=a, max_len=b, seed_len=s, max_mm_seed=ms,
                                      max_mm_total=mt, trim5=t5, trim3=t3, poly_t=pt)
                                 for (k, a, b, s, ms, mt, t5, t3, pt) in rows])

    def make_passes(self, rows):
        arr = (PassCfg * len(rows))()
        for i, r in enumerate(rows):
            lib = r["lib"]
            arr[i].lib = self.libs[lib] if isinstance(lib, str) else int(lib)
            arr[i].seed_len = int(r.get("seed_len", 28))
            arr[i].max_mm_seed = int(r.get("max_mm_seed", 0))
            arr[i].max_mm_total = int(r.get("max_mm_total", 2))
            arr[i].trim5 = int(r.get("trim5", 0))
            arr[i].trim3 = int(r.get("trim3", 0))
            arr[i].min_len = int(r.get("min_len", 0))
            arr[i].max_len = int(r.get("max_len", 255))
            arr[i].poly_t = int(r.get("poly_t", 0))
        return arr

    # ------------------------------------------------------------------
    def _stream_ptr(self):
        torch = _torch()
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _dev(self, x, np_dtype, view=None):
        """None or a device tensor as it is; a host array as np_dtype (its bits seen as `view`) on the device."""
        torch = _torch()
        if x is None or torch.is_tensor(x):
            return x
        a = np.ascontiguousarray(x, dtype=np_dtype)
        return torch.from_numpy(a if view is None else a.view(view)).to(self.device)

    def _dev_reads(self, words, lens, nmask):
        """words [W, n] / lens / nmask (or None) of a read set, contiguous on the device."""
        words = self._dev(words, np.uint64, np.int64).contiguous()
        nmask = self._dev(nmask, np.uint64, np.int64)
        if nmask is not None:
            nmask = nmask.contiguous()
        return words, self._dev(lens, np.uint8).contiguous(), nmask

    def _tmp(self, sizer, *sizes, floor=0):
        """A stage's scratch: the bytes `sizer` (a mrg_*_temp_bytes call of one output) reports for `sizes`, at least
        `floor`, as a uint8 device tensor.  The one place where stage scratch is allocated."""
        torch = _torch()
        need = C.c_uint64()
        check(sizer(*[int(s) for s in sizes], C.byref(need)))
        return torch.empty(max(int(need.value), floor), dtype=torch.uint8, device=self.device)

    def _predict_tmp(self, n):
        return self._tmp(self._lib.mrg_predict_reads_temp_bytes, n)

    def _remap_tmp(self, n_reads, n_rows):
        return self._tmp(self._lib.mrg_predict_remap_temp_bytes, n_reads, n_rows, floor=8)

    def _screen_tmp(self, n_cand):
        return self._tmp(self._lib.mrg_predict_screen_temp_bytes, n_cand, floor=64)

    def _order_sizer(self, which):
        """mrg_collapsed_order_temp_bytes as a sizer of one output: 0 = mrg_seq_rank's scratch, 1 = mrg_collapsed_order's."""
        def sizer(n, out):
            other = C.byref(C.c_uint64())
            return self._lib.mrg_collapsed_order_temp_bytes(n, *((out, other) if which == 0 else (other, out)))
        return sizer

    def _workspace(self, n):
        torch = _torch()
        need = C.c_uint64()
        check(self._lib.mrg_cascade_workspace_bytes(n, C.byref(need)))
        if self._ws is None or self._ws.numel() < need.value:
            self._ws = torch.empty(need.value, dtype=torch.uint8, device=self.device)
        return self._ws

    def cascade(self, reads, passes, out=None):
        """Run the cascade on a ReadSet; asynchronous on torch's current stream."""
        torch = _torch()
        n, n_pass = reads.n, len(passes)
        dev = self.device
        if out is None:
            out = (torch.empty(n, dtype=torch.int8, device=dev),
                   torch.empty(n, dtype=torch.int32, device=dev),
                   torch.empty(n, dtype=torch.int32, device=dev),
                   torch.empty(n, dtype=torch.uint8, device=dev),
                   torch.zeros(2 * n_pass, dtype=torch.int64, device=dev))
        pass_id, ref_id, pos, mm, pass_counts = out
        ws = self._workspace(n)
        # the length range of this batch (known on the host): passes whose window excludes it are
        # skipped; set before every run so that a hint never outlives its batch
        self.set_option("hint_min_len", reads.min_len)
        self.set_option("hint_max_len", reads.max_len)
        check(self._lib.mrg_cascade_run(
            self._h, reads.words.data_ptr(), reads.W, reads.lens.data_ptr(),
            reads.nmask.data_ptr() if reads.nmask is not None else None, n, passes, n_pass,
            pass_id.data_ptr(), ref_id.data_ptr(), pos.data_ptr(), mm.data_ptr(),
            pass_counts.data_ptr(), ws.data_ptr(), ws.numel(), self._stream_ptr()))
        return CascadeResult(pass_id, ref_id, pos, mm, pass_counts, self, n_pass)

    def cascade_long(self, seqs, passes, pass_counts=None, stats=None):
        """The cascade for reads of ANY length (mrg_cascade_run_long; RAP:543-554 offers every unannotated read,
        whatever its length, to every pass): `seqs` = ASCII reads the packed batches cannot describe (beyond 255 nt;
        any length works).  Returns host arrays (pass_id int8, ref_id int32, pos int32, mm uint8) and the per-pass
        dicts (processed, aligned, steps, candidates, lookups, ms) of these reads.  pass_counts: the device int64
        [2 n_pass] vector of the batch's own cascade -- the long reads' processed / aligned are ADDED to it;
        stats: the per-pass dicts of that cascade (CascadeResult.stats) -- added to in place.  Synchronises."""
        torch = _torch()
        from . import pack
        n, n_pass = len(seqs), len(passes)
        dev = self.device
        words, nmask, word_off, lens = pack.pack_ragged(list(seqs))

        def up(a, dt):
            return torch.from_numpy(np.ascontiguousarray(a).view(dt)).to(dev) if a is not None else None
        d_words = up(np.append(words, np.uint64(0)), np.int64)   # (one word of padding: an empty batch still has a buffer)
        d_nmask = up(None if nmask is None else np.append(nmask, np.uint64(0)), np.int64)
        d_off, d_lens = up(word_off, np.int64), up(lens, np.int32)
        out = (torch.empty(n, dtype=torch.int8, device=dev), torch.empty(n, dtype=torch.int32, device=dev),
               torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.uint8, device=dev))
        st = (PassStats * n_pass)()
        check(self._lib.mrg_cascade_run_long(
            self._h, d_words.data_ptr(), d_nmask.data_ptr() if d_nmask is not None else None, d_off.data_ptr(),
            d_lens.data_ptr(), n, passes, n_pass, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr(),
            pass_counts.data_ptr() if pass_counts is not None else None, st, self._stream_ptr()))
        own = [dict(processed=int(s.processed), aligned=int(s.aligned), steps=int(s.steps), candidates=int(s.candidates),
                    lookups=int(s.lookups), ms=float(s.ms)) for s in st]
        if stats is not None:
            for mine, theirs in zip(own, stats):
                for k, v in mine.items():
                    theirs[k] += v
        return tuple(t.cpu().numpy() for t in out) + (own,)

    def pack_assignments(self, result, out=None):
        """The four assignment arrays of a CascadeResult as one int32 word per read (mrg_pack_assignments:
        pass + 1 in bits 28-31, mismatches 26-27, entry 8-25, offset 0-7, the last three saturating):
        4 bytes per read to move over PCIe instead of 10.  Asynchronous; returns the device tensor."""
        torch = _torch()
        n = int(result.pass_id.numel())
        if out is None:
            out = torch.empty(n, dtype=torch.int32, device=self.device)
        check(self._lib.mrg_pack_assignments(self._h, result.pass_id.data_ptr(), result.ref_id.data_ptr(), result.pos.data_ptr(),
                                             result.mm.data_ptr(), n, out.data_ptr(), self._stream_ptr()))
        return out

    def prepare(self, passes, words_per_read=1, min_len=0, max_len=255, has_n=False):
        """Build, ahead of the first timed run, whatever a cascade with these passes on batches of this
        shape derives lazily (the index over several small libraries searched with one policy, the
        anchor-pair tables of a large library for reads with short seed regions): a cascade over zero
        reads with the same length hints plans exactly the same launches."""
        torch = _torch()
        W = int(words_per_read)
        rs = ReadSet.from_device(torch.empty((W, 0), dtype=torch.int64, device=self.device),
                                 torch.empty(0, dtype=torch.uint8, device=self.device),
                                 torch.empty((W, 0), dtype=torch.int64, device=self.device) if has_n else None, None,
                                 int(min_len), int(max_len))
        self.cascade(rs, passes)
        torch.cuda.synchronize(self.device)

    def cascade_packed(self, reads, passes, out=None):
        """The cascade with ONE 4-byte word per read as its per-read output (mrg_cascade_run_packed: every
        kernel writes the packed assignment instead of pass_id / ref_id / pos / mm; SURVEY.md 8d's "4 B
        packed assignment out").  out = (packed int32 [n], pass_counts int64 [2 n_pass])."""
        torch = _torch()
        n, n_pass = reads.n, len(passes)
        if out is None:
            out = (torch.empty(n, dtype=torch.int32, device=self.device), torch.zeros(2 * n_pass, dtype=torch.int64, device=self.device))
        packed, pass_counts = out
        ws = self._workspace(n)
        self.set_option("hint_min_len", reads.min_len)
        self.set_option("hint_max_len", reads.max_len)
        check(self._lib.mrg_cascade_run_packed(
            self._h, reads.words.data_ptr(), reads.W, reads.lens.data_ptr(),
            reads.nmask.data_ptr() if reads.nmask is not None else None, n, passes, n_pass, packed.data_ptr(),
            pass_counts.data_ptr(), ws.data_ptr(), ws.numel(), self._stream_ptr()))
        return CascadeResult(None, None, None, None, pass_counts, self, n_pass, packed=packed)

    def _run_id(self):
        v = C.c_uint64()
        check(self._lib.mrg_cascade_run_id(self._h, C.byref(v)))
        return int(v.value)

    def _read_stats(self, n_pass):
        st = (PassStats * n_pass)()
        check(self._lib.mrg_cascade_stats(self._h, st, n_pass))
        return [dict(processed=int(s.processed), aligned=int(s.aligned), steps=int(s.steps),
                     candidates=int(s.candidates), lookups=int(s.lookups), ms=float(s.ms),
                     lds_bytes=int(s.lds_bytes), lds_mode=int(s.lds_mode), group=int(s.group),
                     n_launches=int(s.n_launches), kbits_log2=int(s.kbits_log2),
                     pair_anchor=int(s.pair_anchor), ms_rest=float(s.ms_rest), variant=int(s.variant))
                for s in st]

    def counts_len(self, n_mirna, n_samples, n_pass):
        ln = C.c_uint64()
        check(self._lib.mrg_tally_counts_len(n_mirna, n_samples, n_pass, C.byref(ln)))
        return int(ln.value)

    def tally(self, reads, result, n_mirna, canon_pass=CANON_PASS, isomir_pass=ISOMIR_PASS,
              counts=None):
        """summarize.py:34-66 on device; returns the fused int64 count vector (device)."""
        torch = _torch()
        if reads.quant is None:
            raise ValueError("ReadSet has no quant matrix")
        S = reads.n_samples
        ln = self.counts_len(n_mirna, S, result.n_pass)
        if counts is None:
            counts = torch.zeros(ln, dtype=torch.int64, device=self.device)
        if getattr(result, "packed", None) is not None:
            check(self._lib.mrg_tally_run_packed(
                self._h, result.packed.data_ptr(), reads.quant.data_ptr(), reads.n, S, n_mirna, result.n_pass, canon_pass,
                isomir_pass, counts.data_ptr(), self._stream_ptr()))
            return counts
        check(self._lib.mrg_tally_run(
            self._h, result.pass_id.data_ptr(), result.ref_id.data_ptr(), reads.quant.data_ptr(),
            reads.n, S, n_mirna, result.n_pass, canon_pass, isomir_pass, counts.data_ptr(),
            self._stream_ptr()))
        return counts

    # ---- torch-less multi-GPU (the C-ABI's own RCCL binding; mirge_amd.dist uses torch.distributed)
    @staticmethod
    def comm_unique_id():
        buf = C.create_string_buffer(128)
        check(_native.load().mrg_comm_unique_id(buf))
        return buf.raw

    def comm_init(self, unique_id, rank, world):
        check(self._lib.mrg_comm_init(self._h, C.c_char_p(bytes(unique_id)), int(rank), int(world)))

    def allreduce(self, counts):
        """In-place uint64 sum of a device tensor (int64 storage) over the ranks of comm_init."""
        check(self._lib.mrg_allreduce(self._h, counts.data_ptr(), counts.numel(), self._stream_ptr()))
        return counts

    def comm_destroy(self):
        check(self._lib.mrg_comm_destroy(self._h))

    EDIT_POSITIONS = 32

    def edit_counts_len(self, lib, n_samples, n_bins=None):
        ln = C.c_uint64()
        nb = self.indexes[lib].n_ref if n_bins is None else int(n_bins)
        check(self._lib.mrg_edit_counts_len(nb, int(n_samples), C.byref(ln)))
        return int(ln.value)

    def edit_tally(self, reads, result, lib="mirna", canon_pass=CANON_PASS, isomir_pass=ISOMIR_PASS, counts=None,
                   keep=None, remap=None, n_bins=None, from_base=0, to_base=2, isomir_trim5=1, flank5=2, flank3=6):
        """The per-read part of A2IEditing (writeDataToCSV.py:145-229) on device: per (miRNA bin, sample)
        count_true / seq_true / canonical and, per mature position, the counts of kept reads showing
        `to_base` where the mature sequence has `from_base` (A -> G by default).  keep: uint8 device
        tensor [n] or None; remap: int32 device tensor [entries] -> bin or None.  Returns the int64
        device vector laid out as mrg_edit_tally_run documents (split with split_edit_counts)."""
        torch = _torch()
        S = reads.n_samples
        nb = self.indexes[lib].n_ref if n_bins is None else int(n_bins)
        ln = self.edit_counts_len(lib, S, nb)
        if counts is None:
            counts = torch.zeros(ln, dtype=torch.int64, device=self.device)
        if getattr(result, "packed", None) is not None:
            check(self._lib.mrg_edit_tally_run_packed(
                self._h, reads.words.data_ptr(), reads.W, reads.lens.data_ptr(),
                reads.nmask.data_ptr() if reads.nmask is not None else None, result.packed.data_ptr(), reads.quant.data_ptr(),
                None if keep is None else keep.data_ptr(), None if remap is None else remap.data_ptr(), reads.n, S, nb,
                self.libs[lib], canon_pass, isomir_pass, isomir_trim5, flank5, flank3, from_base, to_base,
                counts.data_ptr(), self._stream_ptr()))
            return counts
        check(self._lib.mrg_edit_tally_run(
            self._h, reads.words.data_ptr(), reads.W, reads.lens.data_ptr(),
            reads.nmask.data_ptr() if reads.nmask is not None else None, result.pass_id.data_ptr(),
            result.ref_id.data_ptr(), result.pos.data_ptr(), reads.quant.data_ptr(),
            None if keep is None else keep.data_ptr(), None if remap is None else remap.data_ptr(), reads.n, S, nb,
            self.libs[lib], canon_pass, isomir_pass, isomir_trim5, flank5, flank3, from_base, to_base,
            counts.data_ptr(), self._stream_ptr()))
        return counts

    def last_tally_launch(self, edit=False):
        """Which instantiation the last tally (edit=True: edit tally) launch of this engine ran
        (mrg_ctx_last_tally_launch): dict(lds_hist, lds_lib, vec4, grid, lds_bytes)."""
        out = (C.c_uint32 * 4)()
        which = _native.MRG_TALLY_LAUNCH_EDIT if edit else _native.MRG_TALLY_LAUNCH_COUNTS
        check(self._lib.mrg_ctx_last_tally_launch(self._h, which, out))
        return dict(lds_hist=bool(out[0] & _native.MRG_TALLY_LDS_HIST), lds_lib=bool(out[0] & _native.MRG_TALLY_LDS_LIB),
                    vec4=bool(out[0] & _native.MRG_TALLY_VEC4), grid=int(out[1]), lds_bytes=int(out[2]))

    def collapse(self, words, lens, nmask=None, sample=None, n_samples=1, max_len=0, out=None):
        """quantReads (QNT:3-24) on device tensors: raw reads (words int64 [W, n], lens uint8 [n],
        nmask or None, sample int16 [n] or None) -> (ReadSet of the unique reads with their
        per-sample counts, all still in HBM and ordered by (length, bases); read-length histogram
        int64 [256, S]).  Synchronises (the number of uniques comes back to the host).
        out = (u_words [W, n], u_lens [n], u_nmask or None, quant [n, S]): caller-owned output
        buffers (a pipeline that collapses batch after batch keeps one set instead of asking the
        allocator for n-sized arrays every time)."""
        torch = _torch()
        dev = self.device
        W, n = int(words.shape[0]), int(words.shape[1])
        cap = max(n, 1)
        if out is not None:
            u_words, u_lens, u_nmask, quant = out
            if tuple(u_words.shape) != (W, cap) or u_lens.numel() != cap or tuple(quant.shape) != (cap, n_samples) or \
                    (nmask is not None and u_nmask is None):
                raise ValueError("collapse: output buffers do not match the input shape")
        else:
            u_words = torch.empty((W, cap), dtype=torch.int64, device=dev)
            u_lens = torch.empty(cap, dtype=torch.uint8, device=dev)
            u_nmask = None if nmask is None else torch.empty((W, cap), dtype=torch.int64, device=dev)
            quant = torch.empty((cap, n_samples), dtype=torch.int32, device=dev)
        hist = torch.zeros((256, n_samples), dtype=torch.int64, device=dev)
        n_unique = C.c_uint64(0)
        check(self._lib.mrg_collapse_run(
            self._h, words.data_ptr(), W, lens.data_ptr(), None if nmask is None else nmask.data_ptr(),
            None if sample is None or n_samples == 1 else sample.data_ptr(), n, n_samples, int(max_len), cap,
            u_words.data_ptr(), u_lens.data_ptr(), None if u_nmask is None else u_nmask.data_ptr(),
            quant.data_ptr(), hist.data_ptr(), C.byref(n_unique), self._stream_ptr()))
        U = int(n_unique.value)
        # the SoA stride of the cascade is the array's own row length: compact views
        rs = ReadSet.from_device(u_words[:, :U].contiguous() if U != cap else u_words, u_lens[:U],
                                 None if u_nmask is None else (u_nmask[:, :U].contiguous() if U != cap else u_nmask),
                                 quant[:U], 0, int(max_len) if max_len else 255)
        return rs, hist

    def last_collapse(self):
        """What the last collapse of this engine that succeeded did (mrg_ctx_last_collapse): dict(path, reason, n_chunks,
        chunk, n_hot, n_pairs, n_buckets, n_unique).  path 0 = general path, fast path not tried; 1 = the fast path
        answered; 2 = it declined the batch's shape after its prepass; 3 = one of its reduce tables overflowed (2 and 3:
        the general path answered).  reason says why for paths 0 and 2 (include/mirge_amd.h lists the values)."""
        out = (C.c_uint32 * 8)()
        check(self._lib.mrg_ctx_last_collapse(self._h, out))
        return dict(zip(("path", "reason", "n_chunks", "chunk", "n_hot", "n_pairs", "n_buckets", "n_unique"), (int(x) for x in out)))

    def expand_compact(self, bits, runs, quant8=None, esc=None, n_samples=1, out=None):
        """mrg_expand_compact: the compact wire form of a host-resident collapsed read set
        (pack.compact_read_set; bits int64 [n_words] and quant8 uint8 [n, S] / esc int32 [k, 2] already on
        the device, runs a host array of (length, count)) -> ReadSet in HBM.  Asynchronous.
        out = (words int64 [1, n], lens uint8 [n], quant int32 [n, S] or None): caller-owned buffers."""
        torch = _torch()
        dev = self.device
        runs = np.ascontiguousarray(np.asarray(runs, dtype=np.uint32).reshape(-1, 2))
        n = int(runs[:, 1].sum())
        if out is not None:
            words, lens, quant = out
        else:
            words = torch.empty((1, max(n, 1)), dtype=torch.int64, device=dev)[:, :n]
            lens = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)[:n]
            quant = None if quant8 is None else torch.empty((max(n, 1), n_samples), dtype=torch.int32, device=dev)[:n]
        check(self._lib.mrg_expand_compact(
            self._h, bits.data_ptr(), int(bits.numel()), runs.ctypes.data, runs.shape[0], None if quant8 is None else quant8.data_ptr(),
            None if esc is None or esc.shape[0] == 0 else esc.data_ptr(), 0 if esc is None else int(esc.shape[0]), n, n_samples,
            words.data_ptr(), lens.data_ptr(), None if quant8 is None else quant.data_ptr(), self._stream_ptr()))
        live = runs[:, 0][runs[:, 1] > 0]
        return ReadSet.from_device(words, lens, None, None if quant8 is None else quant, int(live.min()) if n else 0,
                                   int(live.max()) if n else 255)

    def count_best(self, reads, lib, seed_len=28, max_mm_seed=1, max_mm_total=2):
        """Best stratum of every read of a ReadSet against one library, forward strand:
        (fewest mismatches or 255, alignments reaching it, saturating) as host uint8 arrays.
        The -ai genome filters of writeDataToCSV.py:1263/:1488 (see mirge_amd.a2i)."""
        torch = _torch()
        mm = torch.empty(reads.n, dtype=torch.uint8, device=self.device)
        cnt = torch.empty(reads.n, dtype=torch.uint8, device=self.device)
        lid = self.libs[lib] if isinstance(lib, str) else int(lib)
        check(self._lib.mrg_count_best(
            self._h, reads.words.data_ptr(), reads.W, reads.lens.data_ptr(),
            reads.nmask.data_ptr() if reads.nmask is not None else None, reads.n, lid, int(seed_len),
            int(max_mm_seed), int(max_mm_total), mm.data_ptr(), cnt.data_ptr(), self._stream_ptr()))
        return mm.cpu().numpy(), cnt.cpu().numpy()

    def list_best(self, reads, lib, seed_len=28, max_mm_seed=0, max_mm_total=0):
        """`-a --best --strata` (RAP:577-599; parseAlignment3 RAP:41-52): every alignment of each
        read's best stratum.  Returns host arrays (best_mm[n], offsets[n+1], ref[total],
        pos[total]); read r owns ref/pos[offsets[r]:offsets[r+1]], sorted by (entry, offset)."""
        torch = _torch()
        n = reads.n
        mm = torch.empty(n, dtype=torch.uint8, device=self.device)
        off = torch.empty(n + 1, dtype=torch.int64, device=self.device)
        lid = self.libs[lib] if isinstance(lib, str) else int(lib)
        nm = reads.nmask.data_ptr() if reads.nmask is not None else None
        total = C.c_uint64(0)
        check(self._lib.mrg_list_best_count(
            self._h, reads.words.data_ptr(), reads.W, reads.lens.data_ptr(), nm, n, lid, int(seed_len),
            int(max_mm_seed), int(max_mm_total), mm.data_ptr(), off.data_ptr(), C.byref(total),
            self._stream_ptr()))
        t = int(total.value)
        ref = torch.empty(max(t, 1), dtype=torch.int32, device=self.device)
        pos = torch.empty(max(t, 1), dtype=torch.int32, device=self.device)
        check(self._lib.mrg_list_best_fill(
            self._h, reads.words.data_ptr(), reads.W, reads.lens.data_ptr(), nm, n, lid, int(seed_len),
            int(max_mm_seed), int(max_mm_total), mm.data_ptr(), off.data_ptr(), t, ref.data_ptr(),
            pos.data_ptr(), self._stream_ptr()))
        off_h = off.cpu().numpy()
        ref_h, pos_h = ref.cpu().numpy()[:t], pos.cpu().numpy()[:t]
        # canonical order inside each read: (entry, offset)
        owner = np.repeat(np.arange(n, dtype=np.int64), np.diff(off_h))
        order = np.lexsort((pos_h, ref_h, owner))
        return mm.cpu().numpy(), off_h, ref_h[order], pos_h[order]

    def isomir_classify(self, table, words, lens, nmask, pass_id, ref_id, pos, canon_pass=CANON_PASS,
                        isomir_pass=ISOMIR_PASS, timings=None):
        """The rows of the `-gff` files (mrg_isomir_classify): the reads claimed by canon_pass in array order, then those
        claimed by isomir_pass, each classified against its entry of `table` (isomir.entry_table).  words [W, n] / lens /
        nmask (or None) / pass_id / ref_id / pos: the device tensors of a ReadSet and a CascadeResult, or host arrays
        (uploaded).  Returns host arrays (idx uint32 [k], rec int32 [k, 8], mask uint64 [k, ceil(W / 2)], rows of the
        canon pass, rows of the isomiR pass).  timings: a dict that receives `kernel_ms`, the time of classify_kernel alone (device events
        inside the call), and `classify_call_ms`, the whole filling call (selection, table uploads, kernel; events around it).
        The rows are counted by a first call and filled by a second: the selection (two launches and a scan) runs twice."""
        torch = _torch()
        words, lens, nmask = self._dev_reads(words, lens, nmask)
        pass_id = self._dev(pass_id, np.int8).contiguous()
        ref_id, pos = self._dev(ref_id, np.int32).contiguous(), self._dev(pos, np.int32).contiguous()
        W, n = int(words.shape[0]), int(words.shape[1])
        desc = np.ascontiguousarray(table.desc, dtype=np.int32)
        text = np.ascontiguousarray(table.words, dtype=np.uint64)
        npl = np.ascontiguousarray(table.nplane, dtype=np.uint64)
        counts = (C.c_uint64 * 2)()

        kernel_ms = C.c_float(0.0)

        def call(cap, idx, rec, mask):
            check(self._lib.mrg_isomir_classify(
                self._h, words.data_ptr(), W, n, lens.data_ptr(), None if nmask is None else nmask.data_ptr(), n,
                pass_id.data_ptr(), ref_id.data_ptr(), pos.data_ptr(), int(canon_pass), int(isomir_pass), desc.ctypes.data,
                desc.shape[0], text.ctypes.data, npl.ctypes.data, text.shape[0], cap,
                None if idx is None else idx.data_ptr(), None if rec is None else rec.data_ptr(),
                None if mask is None else mask.data_ptr(), counts, None if timings is None else C.byref(kernel_ms),
                self._stream_ptr()))
        call(0, None, None, None)
        k = int(counts[0]) + int(counts[1])
        mw = (W + 1) // 2
        idx = torch.empty(max(k, 1), dtype=torch.int32, device=self.device)
        rec = torch.empty((max(k, 1), 8), dtype=torch.int32, device=self.device)
        mask = torch.empty((max(k, 1), mw), dtype=torch.int64, device=self.device)
        if k:
            with _timed(timings, "classify_call_ms"):
                call(k, idx, rec, mask)
            if timings is not None:
                timings["kernel_ms"] = float(kernel_ms.value)
        return (idx.cpu().numpy().view(np.uint32)[:k], rec.cpu().numpy()[:k], mask.cpu().numpy().view(np.uint64)[:k],
                int(counts[0]), int(counts[1]))

    def a2i_align(self, table, words, lens, nmask, pass_id, ref_id, keep=None, timings=None, from_base="A", to_base="G",
                  canon_pass=CANON_PASS, isomir_pass=ISOMIR_PASS, settle=False):
        """The rows of the `-ai` report (mrg_a2i_align): the reads claimed by canon_pass or isomir_pass (and, where `keep`
        is given, with keep != 0), in array order, each aligned to the canonical sequence of its miRNA in `table`
        (a2i.target_table).  words [W, n] / lens / nmask (or None) / pass_id / ref_id / keep: the device tensors of a
        ReadSet and a CascadeResult, or host arrays (uploaded).  Returns host arrays (idx uint32 [k], rec int32 [k, 4]:
        status | verdict << 8 | substring << 9 | m << 16, the diagonal, the edit mask, the target id).  timings: a dict that
        receives `kernel_ms`, the time of the alignment kernel alone (device events inside the call), and `align_call_ms`,
        the whole filling call.  The rows are counted by a first call and filled by a second.
        settle: before the download, mrg_a2i_settle walks the rows of status 1 (a tie between diagonals) on the device
        and rewrites those it settles as status 5, filled as a row of status 0; timings then also receives
        `settle_examined`, `settle_settled` and `settle_kernel_ms`."""
        torch = _torch()
        from .a2i import BASE_CODE
        words, lens, nmask = self._dev_reads(words, lens, nmask)
        pass_id, ref_id = self._dev(pass_id, np.int8).contiguous(), self._dev(ref_id, np.int32).contiguous()
        if keep is not None:
            keep = (keep.to(torch.uint8) if torch.is_tensor(keep) else self._dev(np.asarray(keep) != 0, np.uint8)).contiguous()
        W, n = int(words.shape[0]), int(words.shape[1])
        canon_t = np.ascontiguousarray(table.by_pass[canon_pass], dtype=np.int32)
        iso_t = np.ascontiguousarray(table.by_pass[isomir_pass], dtype=np.int32)
        t_words = np.ascontiguousarray(table.words, dtype=np.uint64)
        t_lens = np.ascontiguousarray(table.lens, dtype=np.uint8)
        counts = (C.c_uint64 * 1)()
        kernel_ms = C.c_float(0.0)

        def call(cap, idx, rec):
            check(self._lib.mrg_a2i_align(
                self._h, words.data_ptr(), W, n, lens.data_ptr(), None if nmask is None else nmask.data_ptr(), n,
                pass_id.data_ptr(), ref_id.data_ptr(), None if keep is None else keep.data_ptr(), int(canon_pass),
                int(isomir_pass), canon_t.ctypes.data, canon_t.shape[0], iso_t.ctypes.data, iso_t.shape[0],
                t_words.ctypes.data, t_lens.ctypes.data, t_lens.shape[0], BASE_CODE[from_base], BASE_CODE[to_base], cap,
                None if idx is None else idx.data_ptr(), None if rec is None else rec.data_ptr(), counts,
                None if timings is None else C.byref(kernel_ms), self._stream_ptr()))
        call(0, None, None)
        k = int(counts[0])
        idx = torch.empty(max(k, 1), dtype=torch.int32, device=self.device)
        rec = torch.empty((max(k, 1), 4), dtype=torch.int32, device=self.device)
        if k:
            with _timed(timings, "align_call_ms"):
                call(k, idx, rec)
            if timings is not None:
                timings["kernel_ms"] = float(kernel_ms.value)
        if settle:
            done = (C.c_uint64 * 2)()
            settle_ms = C.c_float(0.0)
            if k:
                check(self._lib.mrg_a2i_settle(
                    self._h, words.data_ptr(), W, n, lens.data_ptr(), None if nmask is None else nmask.data_ptr(), n,
                    canon_t.ctypes.data, canon_t.shape[0], iso_t.ctypes.data, iso_t.shape[0], t_words.ctypes.data,
                    t_lens.ctypes.data, t_lens.shape[0], BASE_CODE[from_base], BASE_CODE[to_base], k, idx.data_ptr(),
                    rec.data_ptr(), done, None if timings is None else C.byref(settle_ms), self._stream_ptr()))
            if timings is not None:
                timings.update(settle_examined=int(done[0]), settle_settled=int(done[1]),
                               settle_kernel_ms=float(settle_ms.value))
        return idx.cpu().numpy().view(np.uint32)[:k], rec.cpu().numpy()[:k]

    def trf_classify(self, et, words, lens, nmask, pass_id, mature_pass=2, trailer_pass=3, mature_lib="mature_trna",
                     pre_lib="pre_trna", timings=None):
        """The rows of the `-trf` tables (mrg_trf_classify): the reads claimed by mature_pass in array order, then those
        claimed by trailer_pass, listed against their library on the device (`-v 1` / `-v 0`, a trailer read without its T
        tail), every kept alignment typed, the read's tRNA selected and its predefined tRF assigned against `et`
        (trf.entry_tables over the names of the two libraries).  words [W, n] / lens / nmask (or None) / pass_id: the device
        tensors of a ReadSet and a CascadeResult, or host arrays (uploaded).  Returns host arrays (rec int32 [k, 12], hits
        int32 [h, 4], rows of the mature pass, rows of the trailer pass).  timings: a dict that receives `type_kernel_ms` and
        `assign_kernel_ms` (device events inside the call) and `classify_call_ms` (events around the filling call).  The
        rows are counted by a first call; the filling call is repeated only if the read set has more than 4 kept
        alignments per read."""
        torch = _torch()
        words, lens, nmask = self._dev_reads(words, lens, nmask)
        pass_id = self._dev(pass_id, np.int8).contiguous()
        W, n = int(words.shape[0]), int(words.shape[1])
        desc = np.ascontiguousarray(et.desc, dtype=np.int32)
        clusters = np.ascontiguousarray(et.clusters, dtype=np.int32)
        text = np.ascontiguousarray(et.words, dtype=np.uint64)
        plane = np.ascontiguousarray(et.plane, dtype=np.uint64)
        counts = (C.c_uint64 * 3)()
        kernel_ms = (C.c_float * 2)()
        lids = [self.libs[x] if isinstance(x, str) else int(x) for x in (mature_lib, pre_lib)]

        def call(cap_rows, cap_hits, rec, hits):
            check(self._lib.mrg_trf_classify(
                self._h, words.data_ptr(), W, n, lens.data_ptr(), None if nmask is None else nmask.data_ptr(), n,
                pass_id.data_ptr(), int(mature_pass), int(trailer_pass), lids[0], lids[1], desc.ctypes.data, desc.shape[0],
                clusters.ctypes.data, clusters.shape[0], text.ctypes.data, plane.ctypes.data, text.shape[0], cap_rows,
                cap_hits, None if rec is None else rec.data_ptr(), None if hits is None else hits.data_ptr(), counts,
                None if timings is None else kernel_ms, self._stream_ptr()))
        call(0, 0, None, None)
        n2, n3 = int(counts[0]), int(counts[1])
        k, h = n2 + n3, 0
        rec = torch.empty((max(k, 1), 12), dtype=torch.int32, device=self.device)
        hits = torch.empty((1, 4), dtype=torch.int32, device=self.device)
        if k:
            cap = 4 * k + 64
            while True:
                hits = torch.empty((cap, 4), dtype=torch.int32, device=self.device)
                with _timed(timings, "classify_call_ms"):
                    call(k, cap, rec, hits)
                if timings is not None:
                    timings["type_kernel_ms"], timings["assign_kernel_ms"] = float(kernel_ms[0]), float(kernel_ms[1])
                h = int(counts[2])
                if h <= cap:
                    break
                cap = h
        return rec.cpu().numpy()[:k], hits.cpu().numpy()[:h], n2, n3

    def trf_sample_groups(self, st, rec, words, lens, nmask, quant, denom, timings=None):
        """The (sample, tRNA) blocks of tRFs.samples.tmp/ (mrg_trf_sample_groups) from the rows of trf_classify IN THE ORDER
        OF THE TSV (columnar.write_trf_tables returns them), `st` = trf.sample_tables, denom[s] = maturetrnaReads +
        pretrnaReads.  rec / words [W, n] / lens / nmask (or None) / quant [n, S]: device tensors or host arrays (uploaded).
        Returns a TrfGroups: the downloaded tables and the device tensors mrg_trf_rho takes.  When an item's entry has no
        template (.no_template_row) or a template exceeds 255 nt (.max_len), only the counts are filled: the caller raises.
        timings: a dict that receives `groups_count_ms` / `groups_fill_ms` (events around the two calls) and
        `items_kernel_ms`, `read_order_kernel_ms`, `row_order_kernel_ms`, `pack_kernel_ms` (events inside the filling call)."""
        torch = _torch()
        words, lens, nmask = self._dev_reads(words, lens, nmask)
        quant = self._dev(quant, np.uint32, np.int32).contiguous()
        rec = self._dev(np.asarray(rec).reshape(-1, 12) if not torch.is_tensor(rec) else rec, np.int32).contiguous()
        W, n = int(words.shape[0]), int(words.shape[1])
        S = int(quant.shape[1]) if quant.dim() == 2 else 1
        k = int(rec.shape[0])
        denom = np.ascontiguousarray(denom, dtype=np.uint64)
        if denom.shape[0] != S or int(quant.shape[0]) != n or int(lens.shape[0]) != n:
            raise ValueError("trf_sample_groups: quant [n, S], lens [n] and denom [S] must match the reads")
        entries = np.ascontiguousarray(st.entries, dtype=np.int32)
        counts = (C.c_uint64 * 8)()
        kernel_ms = (C.c_float * 4)()

        def call(cap_blocks, cap_rows, host, devs):
            ptr = lambda t: None if t is None else t.data_ptr()
            check(self._lib.mrg_trf_sample_groups(
                self._h, words.data_ptr(), W, n, lens.data_ptr(), ptr(nmask), n, quant.data_ptr(), S, rec.data_ptr(), k,
                denom.ctypes.data, entries.ctypes.data, entries.shape[0], int(st.n_names), cap_blocks, cap_rows,
                *[None if a is None else a.ctypes.data for a in host], *[ptr(t) for t in devs], counts,
                None if timings is None else kernel_ms, self._stream_ptr()))

        with _timed(timings, "groups_count_ms"):
            call(0, 0, (None,) * 4, (None,) * 5)
        g = TrfGroups()
        g.n_items, B, G, R = (int(counts[i]) for i in range(4))
        g.max_len, g.has_n = int(counts[4]), bool(counts[5])
        g.no_template_row = None if int(counts[6]) == 0xFFFFFFFF else int(counts[6])
        g.G, g.n = G, R
        g.blocks, g.block_sums = np.zeros((B, 6), dtype=np.int32), np.zeros(B, dtype=np.uint64)
        g.off, g.groups = np.zeros(G + 1, dtype=np.uint32), np.zeros((G, 2), dtype=np.int32)
        g.filled = g.no_template_row is None and g.max_len <= 255
        if not g.filled:
            return g
        Wt = (g.max_len + 31) // 32
        g.codes_d = torch.zeros(Wt * max(R, 1), dtype=torch.int64, device=self.device)
        g.nmask_d = torch.zeros(Wt * max(R, 1), dtype=torch.int64, device=self.device) if g.has_n else None
        g.span_d = torch.zeros(max(R, 1), dtype=torch.int16, device=self.device)
        g.rpm_d = torch.zeros(max(R, 1), dtype=torch.float64, device=self.device)
        rows_d = torch.zeros((max(R, 1), 3), dtype=torch.int32, device=self.device)
        if B:
            with _timed(timings, "groups_fill_ms"):
                call(B, R, (g.blocks, g.block_sums, g.off, g.groups), (g.codes_d, g.nmask_d, g.span_d, g.rpm_d, rows_d))
            if (int(counts[1]), int(counts[2]), int(counts[3])) != (B, G, R):
                raise RuntimeError("trf_sample_groups: the counting and the filling call disagree")
            if timings is not None:
                for key, v in zip(("items_kernel_ms", "read_order_kernel_ms", "row_order_kernel_ms", "pack_kernel_ms"), kernel_ms):
                    timings[key] = float(v)
        g.rows_d = rows_d
        g.rows = rows_d.cpu().numpy()[:R].view(np.uint32)
        return g

    def seq_rank(self, words, lens, nmask, max_len=None):
        """rank[u] = the position of packed read u in ascending Python string order (mrg_seq_rank): a device uint32 tensor
        (int32 storage).  words [W, n] / lens / nmask (or None): device tensors or host arrays (uploaded), n >= 1.
        max_len: a bound on the lengths (None: the longest read, read back from the device)."""
        torch = _torch()
        words, lens, nmask = self._dev_reads(words, lens, nmask)
        W, n = int(words.shape[0]), int(words.shape[1])
        if int(lens.shape[0]) != n or (nmask is not None and tuple(nmask.shape) != (W, n)):
            raise ValueError("seq_rank: words [W, n], lens [n] and nmask [W, n] must match")
        if max_len is None:
            max_len = int(lens.max()) if n else 0
        tmp = self._tmp(self._order_sizer(0), n)
        rank = torch.empty(max(n, 1), dtype=torch.int32, device=self.device)
        check(self._lib.mrg_seq_rank(self._h, words.data_ptr(), W, n, lens.data_ptr(), None if nmask is None else nmask.data_ptr(),
                                     n, int(max_len), rank.data_ptr(), tmp.data_ptr(), tmp.numel(), self._stream_ptr()))
        return rank[:n]

    def collapsed_order(self, words, lens, nmask, quant, timings=None):
        """The order of every sample's <sample>.trim.collapse.fa (mrg_seq_rank once, mrg_collapsed_order per sample column):
        a list of S host uint32 arrays, order[s][k] = the read at line pair k of sample s -- the reads with quant[u, s] > 0 by
        (count, sequence) descending, the sequence as a Python string.  words [W, n] / lens / nmask (or None) / quant [n, S]:
        device tensors or host arrays (uploaded).  timings: a dict that receives `rank_ms` (the string rank, shared by the
        samples) and `order_ms` (all the samples, their downloads included), between device events."""
        torch = _torch()
        words, lens, nmask = self._dev_reads(words, lens, nmask)
        if not torch.is_tensor(quant):
            quant = torch.from_numpy(np.ascontiguousarray(quant, dtype=np.uint32).view(np.int32)).to(self.device)
        quant = quant.contiguous()
        n = int(words.shape[1])
        S = int(quant.shape[1]) if quant.dim() == 2 else 1
        if int(quant.shape[0]) != n or int(lens.shape[0]) != n:
            raise ValueError("collapsed_order: quant [n, S] and lens [n] must match the reads")
        if timings is not None:
            timings.update(rank_ms=0.0, order_ms=0.0)
        if n == 0:
            return [np.zeros(0, dtype=np.uint32) for _ in range(S)]
        marks = _Marks(timings)
        marks.mark()
        rank = self.seq_rank(words, lens, nmask)
        marks.mark()
        tmp = self._tmp(self._order_sizer(1), n)
        order = torch.empty(n, dtype=torch.int32, device=self.device)
        rows = C.c_uint64(0)
        out = []
        for s in range(S):
            check(self._lib.mrg_collapsed_order(self._h, quant.data_ptr(), n, S, s, rank.data_ptr(), order.data_ptr(), n,
                                                C.byref(rows), tmp.data_ptr(), tmp.numel(), self._stream_ptr()))
            out.append(order[:int(rows.value)].cpu().numpy().view(np.uint32))
        marks.mark()
        if timings is not None:
            timings.update(rank_ms=marks.ms(0, 1), order_ms=marks.ms(1, 2))
        return out

    def _dev_u32(self, x, what="the array"):
        """A device tensor as it is, a host array as uint32 in int32 storage on the device."""
        torch = _torch()
        if torch.is_tensor(x):
            return self._expect(x, torch.int32, what).contiguous()
        return torch.from_numpy(np.ascontiguousarray(x, dtype=np.uint32).view(np.int32)).to(self.device)

    @staticmethod
    def _expect(t, dtype, what):
        """The device tensor `t`, or TypeError when its elements are not `dtype`: the kernels read raw memory."""
        if t.dtype != dtype:
            raise TypeError("%s must be a %s tensor, not %s" % (what, dtype, t.dtype))
        return t

    def predict_select(self, pass_id, lens, quant, min_len=16, max_len=25, count_cutoff=2):
        """Predict mode's candidate reads (mrg_predict_select; the rules of convert2Fasta.py over unmapped.csv): of the
        unmapped reads (pass_id < 0) the raw list holds those whose counts sum to 1 or more, the filtered list those with
        min_len <= length <= max_len whose counts sum to count_cutoff or more, both numbered from 1 in array order.
        pass_id [n] / lens [n] / quant [n, S]: device tensors or host arrays (uploaded).  Returns a dict of device tensors
        total (int64 [n], every read's sum), raw_no and sel_no (uint32 in int32 storage [n]: the read's number in the
        list, 0 outside it) and the ints n_raw, n_sel."""
        torch = _torch()
        if not torch.is_tensor(pass_id):
            pass_id = torch.from_numpy(np.ascontiguousarray(pass_id, dtype=np.int8)).to(self.device)
        if not torch.is_tensor(lens):
            lens = torch.from_numpy(np.ascontiguousarray(lens, dtype=np.uint8)).to(self.device)
        pass_id = self._expect(pass_id, torch.int8, "predict_select: pass_id").contiguous()
        lens = self._expect(lens, torch.uint8, "predict_select: lens").contiguous()
        quant = self._dev_u32(quant, "predict_select: quant")
        n = int(lens.shape[0])
        S = int(quant.shape[1]) if quant.dim() == 2 else 1
        if int(quant.shape[0]) != n or int(pass_id.shape[0]) != n:
            raise ValueError("predict_select: pass_id [n], lens [n] and quant [n, S] must match")
        tmp = self._predict_tmp(n)
        total = torch.zeros(max(n, 1), dtype=torch.int64, device=self.device)
        raw_no = torch.zeros(max(n, 1), dtype=torch.int32, device=self.device)
        sel_no = torch.zeros(max(n, 1), dtype=torch.int32, device=self.device)
        n_raw, n_sel = C.c_uint64(0), C.c_uint64(0)
        check(self._lib.mrg_predict_select(self._h, pass_id.data_ptr(), lens.data_ptr(), quant.data_ptr(), n, S, int(min_len),
                                           int(max_len), int(count_cutoff), total.data_ptr(), raw_no.data_ptr(), sel_no.data_ptr(),
                                           C.byref(n_raw), C.byref(n_sel), tmp.data_ptr(), tmp.numel(), self._stream_ptr()))
        return dict(total=total[:n], raw_no=raw_no[:n], sel_no=sel_no[:n], n_raw=int(n_raw.value), n_sel=int(n_sel.value))

    def predict_sample_reads(self, quant, numbers, sample, threshold):
        """One sample's rows of a list of predict_select (mrg_predict_sample_reads): the reads u with numbers[u] != 0 and
        quant[u, sample] >= threshold, in array order.  numbers: raw_no with threshold 1, or sel_no with the count cutoff.
        quant [n, S] / numbers [n]: device tensors or host arrays.  Returns device tensors (index, number, count), uint32 in
        int32 storage."""
        torch = _torch()
        quant, numbers = self._dev_u32(quant, "predict_sample_reads: quant"), self._dev_u32(numbers, "predict_sample_reads: numbers")
        n = int(numbers.shape[0])
        S = int(quant.shape[1]) if quant.dim() == 2 else 1
        if int(quant.shape[0]) != n:
            raise ValueError("predict_sample_reads: quant [n, S] and numbers [n] must match")
        tmp = self._predict_tmp(n)
        out = [torch.empty(max(n, 1), dtype=torch.int32, device=self.device) for _ in range(3)]
        rows = C.c_uint64(0)
        check(self._lib.mrg_predict_sample_reads(self._h, quant.data_ptr(), n, S, int(sample), numbers.data_ptr(), int(threshold),
                                                 out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), n, C.byref(rows),
                                                 tmp.data_ptr(), tmp.numel(), self._stream_ptr()))
        k = int(rows.value)
        return out[0][:k], out[1][:k], out[2][:k]

    def predict_gather(self, words, lens, nmask, quant, index, sample=None):
        """The reads index[j] as a compact packed set (mrg_predict_gather), what ReadSet.from_device and cluster_valid take:
        device tensors (words [W, k], lens [k], nmask [W, k] or None, counts [k] uint32 in int32 storage), counts = the
        reads' counts in `sample` (None: their totals, which must fit 32 bits).  words / lens / nmask / quant / index:
        device tensors or host arrays."""
        torch = _torch()
        words, lens, nmask = self._dev_reads(words, lens, nmask)
        self._expect(words, torch.int64, "predict_gather: words")
        self._expect(lens, torch.uint8, "predict_gather: lens")
        if nmask is not None:
            self._expect(nmask, torch.int64, "predict_gather: nmask")
        quant, index = self._dev_u32(quant, "predict_gather: quant"), self._dev_u32(index, "predict_gather: index")
        W, n, k = int(words.shape[0]), int(words.shape[1]), int(index.shape[0])
        S = int(quant.shape[1]) if quant.dim() == 2 else 1
        if int(quant.shape[0]) != n or int(lens.shape[0]) != n or (nmask is not None and tuple(nmask.shape) != (W, n)):
            raise ValueError("predict_gather: words [W, n], lens [n], nmask [W, n] and quant [n, S] must match")
        tmp = self._predict_tmp(n)
        o_words = torch.zeros((W, k), dtype=torch.int64, device=self.device)
        o_nmask = None if nmask is None else torch.zeros((W, k), dtype=torch.int64, device=self.device)
        o_lens = torch.zeros(k, dtype=torch.uint8, device=self.device)
        o_counts = torch.zeros(k, dtype=torch.int32, device=self.device)
        check(self._lib.mrg_predict_gather(
            self._h, words.data_ptr(), W, n, lens.data_ptr(), None if nmask is None else nmask.data_ptr(), n, quant.data_ptr(), S,
            0xFFFFFFFF if sample is None else int(sample), index.data_ptr(), k, o_words.data_ptr(), o_lens.data_ptr(),
            None if o_nmask is None else o_nmask.data_ptr(), o_counts.data_ptr(), tmp.data_ptr(), tmp.numel(), self._stream_ptr()))
        return o_words, o_lens, o_nmask, o_counts

    def list_valid(self, reads, libs, strands=2, stratum_mode=STRATUM_ALL, m=0, seed_len=28, max_mm_seed=0,
                   max_mm_total=2, timings=None):
        """The bowtie front end's listing (mrg_list_valid_count / _fill): every valid alignment of each read of a
        ReadSet against the libraries `libs` (keys or ids: the parts of one genome, whose entries are numbered on
        across the parts in this order), on the forward strand (strands=1, --norc) or both (2).  stratum_mode:
        STRATUM_BEST = the read's best stratum over all parts and strands (`--best --strata`), STRATUM_ALL = every
        valid alignment (`-a`).  m > 0: a read whose reportable total (what that mode lists, summed over the parts)
        exceeds m is suppressed and lists nothing (bowtie's -m).
        Returns host arrays (offsets[n+1], entry, offset, strand (0 = +, 1 = -), mm, suppressed[n] bool); read r owns
        [offsets[r], offsets[r+1]), ordered by mismatches ascending, then (entry, offset, strand) DESCENDING.
        timings: a dict, or None; gets the synchronised wall seconds of the count and of the fill sweeps."""
        nm = reads.nmask.data_ptr() if reads.nmask is not None else None
        args = (reads.words.data_ptr(), reads.W, reads.lens.data_ptr(), nm, reads.n)
        policy = (int(seed_len), int(max_mm_seed), int(max_mm_total))

        def count(lid, cnt):
            check(self._lib.mrg_list_valid_count(self._h, *args, lid, int(strands), *policy, cnt.data_ptr(), self._stream_ptr()))

        def fill(lid, best_d, off_d, t, ref, pos, strand, mm):
            check(self._lib.mrg_list_valid_fill(self._h, *args, lid, int(strands), int(stratum_mode), *policy, best_d.data_ptr(),
                                                off_d.data_ptr(), t, ref.data_ptr(), pos.data_ptr(), strand.data_ptr(),
                                                mm.data_ptr(), self._stream_ptr()))
        return self._list_valid_host(reads.n, libs, stratum_mode, m, count, fill, timings)

    def list_valid_long(self, seqs, libs, strands=2, stratum_mode=STRATUM_ALL, m=0, seed_len=28, max_mm_seed=0,
                        max_mm_total=2, timings=None):
        """list_valid for reads of ANY length (mrg_list_valid_long_count / _fill, one wave per read): `seqs` = ASCII reads
        the packed form cannot describe (beyond 255 nt; any length works), packed into the ragged form as cascade_long
        packs them.  Same libraries, policy, `-m` and stratum rules, and exactly list_valid's return tuple and row order."""
        torch = _torch()
        from . import pack
        n = len(seqs)
        words, nmask, word_off, lens = pack.pack_ragged(list(seqs))

        def up(a, dt):
            return torch.from_numpy(np.ascontiguousarray(a).view(dt)).to(self.device) if a is not None else None
        d_words = up(np.append(words, np.uint64(0)), np.int64)   # (one word of padding: an empty batch still has a buffer)
        d_nmask = up(None if nmask is None else np.append(nmask, np.uint64(0)), np.int64)
        d_off, d_lens = up(word_off, np.int64), up(lens, np.int32)
        args = (d_words.data_ptr(), d_nmask.data_ptr() if d_nmask is not None else None, d_off.data_ptr(), d_lens.data_ptr(), n)
        policy = (int(strands), int(seed_len), int(max_mm_seed), int(max_mm_total))

        def count(lid, cnt):
            check(self._lib.mrg_list_valid_long_count(self._h, *args, lid, *policy, cnt.data_ptr(), self._stream_ptr()))

        def fill(lid, best_d, off_d, t, ref, pos, strand, mm):
            check(self._lib.mrg_list_valid_long_fill(self._h, *args, lid, *policy, int(stratum_mode), best_d.data_ptr(),
                                                     off_d.data_ptr(), t, ref.data_ptr(), pos.data_ptr(), strand.data_ptr(),
                                                     mm.data_ptr(), self._stream_ptr()))
        return self._list_valid_host(n, libs, stratum_mode, m, count, fill, timings)

    def _list_valid_host(self, n, libs, stratum_mode, m, count, fill, timings=None):
        """The host half of a listing, whatever form its reads have: count(lid, cnt [4, n] int32) per part -> the best
        stratum, what is reportable and what `-m` suppresses, decided over all parts from the summed counts -> per-part
        offsets -> fill(lid, best_mm, offsets, rows, ref, pos, strand, mm) per part -> the parts' rows merged, entries
        numbered on across `libs`, ordered by mismatches ascending, then (entry, offset, strand) descending."""
        import time
        torch = _torch()
        dev = self.device
        lids = [self.libs[k] if isinstance(k, str) else int(k) for k in libs]
        keys = {v: k for k, v in self.libs.items()}
        bases = np.cumsum([0] + [self.indexes[keys[l]].n_ref for l in lids])
        per_lib = []
        t0 = time.perf_counter()
        for lid in lids:
            cnt = torch.zeros((4, max(n, 1)), dtype=torch.int32, device=dev)
            count(lid, cnt)
            per_lib.append(cnt.cpu().numpy()[:, :n].view(np.uint32).astype(np.int64))
        if timings is not None:
            timings["count_s"] = time.perf_counter() - t0
        tot = np.sum(per_lib, axis=0) if per_lib else np.zeros((4, n), dtype=np.int64)
        aligned = tot.any(axis=0)
        best = np.where(aligned, np.argmax(tot > 0, axis=0), 255)
        cols = np.arange(n)
        if stratum_mode == STRATUM_BEST:
            reportable = np.where(aligned, tot[np.minimum(best, 3), cols], 0)
        else:
            reportable = tot.sum(axis=0)
        suppressed = (reportable > m) if m > 0 else np.zeros(n, dtype=bool)
        write = aligned & ~suppressed
        best_w = np.where(write, best, 255).astype(np.uint8)
        best_d = torch.from_numpy(best_w if n else np.full(1, 255, np.uint8)).to(dev)
        got = []
        t_fill = 0.0
        for lid, c, base in zip(lids, per_lib, bases):
            k = c[np.minimum(best, 3), cols] if stratum_mode == STRATUM_BEST else c.sum(axis=0)
            k = np.where(write, k, 0)
            off = np.zeros(n + 1, dtype=np.int64)
            np.cumsum(k, out=off[1:])
            t = int(off[-1])
            if t == 0:
                continue
            off_d = torch.from_numpy(off).to(dev)
            ref = torch.empty(t, dtype=torch.int32, device=dev)
            pos = torch.empty(t, dtype=torch.int32, device=dev)
            strand = torch.empty(t, dtype=torch.uint8, device=dev)
            mm = torch.empty(t, dtype=torch.uint8, device=dev)
            t0 = time.perf_counter()
            fill(lid, best_d, off_d, t, ref, pos, strand, mm)
            torch.cuda.current_stream(dev).synchronize()
            t_fill += time.perf_counter() - t0
            got.append((np.repeat(np.arange(n, dtype=np.int64), k), ref.cpu().numpy().astype(np.int64) + int(base),
                        pos.cpu().numpy(), strand.cpu().numpy(), mm.cpu().numpy()))
        if timings is not None:
            timings["fill_s"] = t_fill
        if got:
            owner, entry, pos, strand, mm = (np.concatenate(x) for x in zip(*got))
        else:
            owner, entry = np.zeros(0, np.int64), np.zeros(0, np.int64)
            pos, strand, mm = np.zeros(0, np.int32), np.zeros(0, np.uint8), np.zeros(0, np.uint8)
        order = np.lexsort((-strand.astype(np.int64), -pos.astype(np.int64), -entry, mm, owner))
        offsets = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(np.bincount(owner, minlength=n)[:n], out=offsets[1:])
        return (offsets, entry[order].astype(np.int32), pos[order].astype(np.int32), strand[order], mm[order],
                suppressed)

    def _list_valid_device(self, reads, libs, strands, stratum_mode, m, seed_len, max_mm_seed, max_mm_total, timings=None):
        """list_valid's listing with the offsets and the rows left on the device (mrg_list_valid_count per part, the best
        stratum and `-m` decided over all parts on the host from the counts, mrg_list_valid_fill per part).  Returns a dict:
        bases (first entry number of every part, then the total), n_entries, suppressed [n] bool, n_rows, counts (per part
        the device tensor [4, n] of mrg_list_valid_count), aligned [n] bool; and, unless n_rows is 0, the device tensors ref
        (the part's own entry numbers) / pos / strand / mm [n_rows], part after part, and offsets = per part (int64 [n + 1]
        inside the part's rows, first row, rows).  ValueError beyond 2^32 - 2 rows.  timings gets count_s / fill_s."""
        import time
        torch = _torch()
        n = reads.n
        dev = self.device
        st = self._stream_ptr()
        lids = [self.libs[k] if isinstance(k, str) else int(k) for k in libs]
        keys = {v: k for k, v in self.libs.items()}
        bases = np.cumsum([0] + [self.indexes[keys[l]].n_ref for l in lids])
        nm = reads.nmask.data_ptr() if reads.nmask is not None else None
        args = (reads.W, reads.lens.data_ptr(), nm, n)
        per_lib, counts_d = [], []
        t0 = time.perf_counter()
        for lid in lids:
            cnt = torch.zeros((4, max(n, 1)), dtype=torch.int32, device=dev)
            check(self._lib.mrg_list_valid_count(self._h, reads.words.data_ptr(), *args, lid, int(strands), int(seed_len),
                                                 int(max_mm_seed), int(max_mm_total), cnt.data_ptr(), st))
            per_lib.append(cnt.cpu().numpy()[:, :n].view(np.uint32).astype(np.int64))
            counts_d.append(cnt)
        if timings is not None:
            timings["count_s"] = time.perf_counter() - t0
        tot = np.sum(per_lib, axis=0) if per_lib else np.zeros((4, n), dtype=np.int64)
        aligned = tot.any(axis=0)
        best = np.where(aligned, np.argmax(tot > 0, axis=0), 255)
        cols = np.arange(n)
        if stratum_mode == STRATUM_BEST:
            reportable = np.where(aligned, tot[np.minimum(best, 3), cols], 0)
        else:
            reportable = tot.sum(axis=0)
        suppressed = (reportable > m) if m > 0 else np.zeros(n, dtype=bool)
        write = aligned & ~suppressed
        part_off = []
        for c in per_lib:
            k = c[np.minimum(best, 3), cols] if stratum_mode == STRATUM_BEST else c.sum(axis=0)
            off = np.zeros(n + 1, dtype=np.int64)
            np.cumsum(np.where(write, k, 0), out=off[1:])
            part_off.append(off)
        T = int(sum(int(o[-1]) for o in part_off))
        if T >= 2 ** 32 - 1:
            raise ValueError("%d alignment rows; the limit is 2^32 - 2" % T)
        out = dict(bases=bases, n_entries=int(bases[-1]), suppressed=suppressed, n_rows=T, counts=counts_d, aligned=aligned)
        if T == 0:
            return out

        def dev_empty(count, dtype):
            return torch.empty(max(int(count), 1), dtype=dtype, device=dev)
        best_d = torch.from_numpy(np.where(write, best, 255).astype(np.uint8)).to(dev)
        ref, pos = dev_empty(T, torch.int32), dev_empty(T, torch.int32)
        strand, mm = dev_empty(T, torch.uint8), dev_empty(T, torch.uint8)
        t_fill, row_base, offs_d = 0.0, 0, []
        for lid, off in zip(lids, part_off):
            t = int(off[-1])
            offs_d.append((torch.from_numpy(off).to(dev), row_base, t))
            if t:
                sl = slice(row_base, row_base + t)
                t0 = time.perf_counter()
                check(self._lib.mrg_list_valid_fill(self._h, reads.words.data_ptr(), *args, lid, int(strands), int(stratum_mode),
                                                    int(seed_len), int(max_mm_seed), int(max_mm_total), best_d.data_ptr(),
                                                    offs_d[-1][0].data_ptr(), t, ref[sl].data_ptr(), pos[sl].data_ptr(),
                                                    strand[sl].data_ptr(), mm[sl].data_ptr(), st))
                torch.cuda.current_stream(dev).synchronize()
                t_fill += time.perf_counter() - t0
            row_base += t
        if timings is not None:
            timings["fill_s"] = t_fill
        out.update(ref=ref, pos=pos, strand=strand, mm=mm, offsets=offs_d)
        return out

    def cluster_valid(self, reads, libs, counts, entry_keep=None, threshold=14, strands=2, stratum_mode=STRATUM_ALL, m=0,
                      seed_len=28, max_mm_seed=0, max_mm_total=2, sorted_rows=False, timings=None, keep_device=False):
        """Predict mode's location clusters of the listing of list_valid (same reads, libraries, entry numbering and
        policy; `-m` and the best stratum are decided over all parts from the per-read counts, as there), without the
        alignment rows leaving the device: mrg_list_valid_fill per part, then mrg_cluster_keys / _sort / _scan /
        _bounds / _assemble (the rule is documented there).  counts: uint32 [n], the copies each read stands for;
        entry_keep: bool per entry over all parts (None = all), False drops the entry's alignments from the clusters
        (the reference keeps names containing "chr").
        Returns a dict of host arrays: entry, strand, start, end (1-based inclusive), seq_off [C + 1], seq (bytes),
        count_sum (uint64), member_off [C + 1], members (read numbers, cluster after cluster in list order), suppressed
        [n] bool, n_rows, n_valid (rows on kept entries); clusters are ordered by (entry, strand, start).
        sorted_rows=True adds "rows" = (read, entry, offset, strand, mm) of every alignment ordered by (entry, offset,
        strand, read) -- a coordinate-sorted SAM file's order.  timings: a dict, or None; gets count_s / fill_s as
        list_valid does and the device milliseconds sort_ms / scan_ms / assemble_ms.
        keep_device=True adds "device": the cluster arrays as device tensors for predict_trim (entry, strand, start, end,
        seq_off, seq, and the ints n_clusters, total_len), None when there is no alignment row."""
        torch = _torch()
        n = reads.n
        dev = self.device
        st = self._stream_ptr()
        if int(threshold) < 1:
            raise ValueError("the overlap threshold must be at least 1 (got %d)" % int(threshold))
        nm = reads.nmask.data_ptr() if reads.nmask is not None else None
        ls = self._list_valid_device(reads, libs, strands, stratum_mode, m, seed_len, max_mm_seed, max_mm_total, timings)
        bases, n_entries, suppressed, T = ls["bases"], ls["n_entries"], ls["suppressed"], ls["n_rows"]
        out = dict(suppressed=suppressed, n_rows=T, n_valid=0, entry=np.zeros(0, np.uint32), strand=np.zeros(0, np.uint8),
                   start=np.zeros(0, np.uint32), end=np.zeros(0, np.uint32), seq_off=np.zeros(1, np.uint64), seq=b"",
                   count_sum=np.zeros(0, np.uint64), member_off=np.zeros(1, np.uint32), members=np.zeros(0, np.uint32))
        if sorted_rows:
            out["rows"] = (np.zeros(0, np.uint32), np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.uint8),
                           np.zeros(0, np.uint8))
        if keep_device:
            out["device"] = None
        if T == 0:
            return out

        def dev_empty(count, dtype):
            return torch.empty(max(int(count), 1), dtype=dtype, device=dev)
        ref, pos, strand, mm, offs_d = ls["ref"], ls["pos"], ls["strand"], ls["mm"], ls["offsets"]
        max_pos = int(pos[:T].max())
        if max_pos < 0 or max_pos >= 2 ** 31:
            raise ValueError("an alignment at offset %d; positions must be below 2^31" % max_pos)
        pos_bits = max(1, max_pos.bit_length())
        bits = pos_bits + 1 + max(1, n_entries.bit_length())   # (entry numbers run to n_entries: the masked rows)
        if bits > 64:
            raise ValueError("%d entries do not fit the key's %d entry bits" % (n_entries, 63 - pos_bits))
        counts_d = torch.from_numpy(np.ascontiguousarray(counts, dtype=np.uint32).view(np.int32)).to(dev)
        keep_d = None
        if entry_keep is not None:
            keep = np.ascontiguousarray(entry_keep, dtype=np.uint8)
            if keep.shape != (n_entries,):
                raise ValueError("entry_keep must have one flag per entry (%d)" % n_entries)
            keep_d = torch.from_numpy(keep).to(dev)
        tmp_b, work_b = C.c_uint64(), C.c_uint64()
        check(self._lib.mrg_cluster_workspace_bytes(T, C.byref(tmp_b), C.byref(work_b)))
        tmp = dev_empty(tmp_b.value, torch.uint8)
        work = dev_empty(work_b.value, torch.uint8)
        owner = dev_empty(T, torch.int32)

        def sorted_pairs(order, keep_ptr):
            k0, k1 = dev_empty(T, torch.int64), dev_empty(T, torch.int64)
            v0, v1 = dev_empty(T, torch.int32), dev_empty(T, torch.int32)
            for (off_d, base_row, t), ebase in zip(offs_d, bases):
                if t:
                    sl = slice(base_row, base_row + t)
                    check(self._lib.mrg_cluster_keys(self._h, off_d.data_ptr(), n, ref[sl].data_ptr(), pos[sl].data_ptr(),
                                                     strand[sl].data_ptr(), t, base_row, T, int(ebase), n_entries, pos_bits, order,
                                                     keep_ptr, k0.data_ptr(), v0.data_ptr(), owner.data_ptr(), st))
            second = C.c_int32(0)
            check(self._lib.mrg_cluster_sort(self._h, k0.data_ptr(), k1.data_ptr(), v0.data_ptr(), v1.data_ptr(), T, bits,
                                             tmp.data_ptr(), tmp_b.value, C.byref(second), st))
            return (k1, v1) if second.value else (k0, v0)

        marks = _Marks(timings, dev)
        marks.mark()
        skeys, svals = sorted_pairs(0, keep_d.data_ptr() if keep_d is not None else None)
        marks.mark()
        member = dev_empty(T, torch.int32)
        n_valid, n_clusters = C.c_uint64(), C.c_uint64()
        check(self._lib.mrg_cluster_scan(self._h, skeys.data_ptr(), svals.data_ptr(), T, owner.data_ptr(), reads.lens.data_ptr(),
                                         n_entries, pos_bits, int(threshold), work.data_ptr(), work_b.value, tmp.data_ptr(),
                                         tmp_b.value, member.data_ptr(), C.byref(n_valid), C.byref(n_clusters), st))
        V, K = int(n_valid.value), int(n_clusters.value)
        c_entry, c_start, c_end = dev_empty(K, torch.int32), dev_empty(K, torch.int32), dev_empty(K, torch.int32)
        c_strand = dev_empty(K, torch.uint8)
        c_moff, c_len, c_soff = dev_empty(K + 1, torch.int32), dev_empty(K + 1, torch.int32), dev_empty(K + 1, torch.int64)
        total = C.c_uint64()
        check(self._lib.mrg_cluster_bounds(self._h, skeys.data_ptr(), T, V, K, pos_bits, work.data_ptr(), work_b.value,
                                           tmp.data_ptr(), tmp_b.value, c_entry.data_ptr(), c_strand.data_ptr(), c_start.data_ptr(),
                                           c_end.data_ptr(), c_moff.data_ptr(), c_len.data_ptr(), c_soff.data_ptr(),
                                           C.byref(total), st))
        marks.mark()
        seq = dev_empty(total.value, torch.uint8)
        c_sum = dev_empty(K, torch.int64)
        check(self._lib.mrg_cluster_assemble(self._h, skeys.data_ptr(), T, V, K, pos_bits, work.data_ptr(), work_b.value,
                                             member.data_ptr(), reads.words.data_ptr(), reads.W, reads.lens.data_ptr(), nm, n,
                                             counts_d.data_ptr(), c_start.data_ptr(), c_soff.data_ptr(), seq.data_ptr(),
                                             c_sum.data_ptr(), st))
        marks.mark()
        out.update(n_valid=V,
                   entry=c_entry.cpu().numpy()[:K].view(np.uint32), strand=c_strand.cpu().numpy()[:K],
                   start=c_start.cpu().numpy()[:K].view(np.uint32), end=c_end.cpu().numpy()[:K].view(np.uint32),
                   seq_off=c_soff.cpu().numpy()[:K + 1].view(np.uint64), seq=seq.cpu().numpy()[:int(total.value)].tobytes(),
                   count_sum=c_sum.cpu().numpy()[:K].view(np.uint64), member_off=c_moff.cpu().numpy()[:K + 1].view(np.uint32),
                   members=member.cpu().numpy()[:V].view(np.uint32))
        if keep_device:
            out["device"] = dict(entry=c_entry, strand=c_strand, start=c_start, end=c_end, seq_off=c_soff, seq=seq, n_clusters=K,
                                 total_len=int(total.value))
        if timings is not None:
            for name, a, b in (("sort_ms", 0, 1), ("scan_ms", 1, 2), ("assemble_ms", 2, 3)):
                timings[name] = marks.ms(a, b)
        if sorted_rows:
            del skeys, svals
            skeys, svals = sorted_pairs(1, None)
            r_read, r_entry, r_pos = dev_empty(T, torch.int32), dev_empty(T, torch.int32), dev_empty(T, torch.int32)
            r_strand, r_mm = dev_empty(T, torch.uint8), dev_empty(T, torch.uint8)
            check(self._lib.mrg_cluster_sorted_rows(self._h, skeys.data_ptr(), svals.data_ptr(), T, pos_bits, 1, owner.data_ptr(),
                                                    mm.data_ptr(), r_read.data_ptr(), r_entry.data_ptr(), r_pos.data_ptr(),
                                                    r_strand.data_ptr(), r_mm.data_ptr(), st))
            out["rows"] = (r_read.cpu().numpy()[:T].view(np.uint32), r_entry.cpu().numpy()[:T], r_pos.cpu().numpy()[:T],
                           r_strand.cpu().numpy()[:T], r_mm.cpu().numpy()[:T])
        return out

    def predict_trim(self, clusters, repeats, cutoff=30, timings=None):
        """Predict mode's preliminary trim of the location clusters (mrg_predict_trim; the rules of preTrimClusteredSeq.py
        and generate_Seq.py).  clusters: the "device" dict of cluster_valid(keep_device=True), or a dict of host arrays
        entry, strand, start, end, seq_off [K + 1], seq (bytes) as cluster_valid returns them (uploaded).  repeats: the
        dict of predict.load_repeats (rep_off [entries + 1], start, end; uploaded once per device).
        Returns a dict: the host arrays flag (uint8 [K]), rep (int32 [K]: the element's index in the table, -1 = `*`),
        orig (bytes), kept (uint32: the retained clusters), kept_seq_off (uint64 [kept + 1]), kept_orig (bytes), and
        "device" with the same as device tensors.  timings: a dict that receives trim_ms (device events) and
        download_ms."""
        torch = _torch()
        dev = self.device
        if "n_clusters" in clusters:
            d = clusters
            K, total = int(d["n_clusters"]), int(d["total_len"])
            self._expect(d["entry"], torch.int32, "predict_trim: entry")
            self._expect(d["strand"], torch.uint8, "predict_trim: strand")
            self._expect(d["start"], torch.int32, "predict_trim: start")
            self._expect(d["end"], torch.int32, "predict_trim: end")
            self._expect(d["seq_off"], torch.int64, "predict_trim: seq_off")
            self._expect(d["seq"], torch.uint8, "predict_trim: seq")
        else:
            K = int(len(clusters["entry"]))
            seq = np.array(np.frombuffer(bytes(clusters["seq"]), dtype=np.uint8))   # (a copy: torch wants writable memory)
            total = int(seq.shape[0])
            soff = np.ascontiguousarray(clusters["seq_off"], dtype=np.uint64)
            if soff.shape != (K + 1,) or any(len(clusters[k]) != K for k in ("strand", "start", "end")):
                raise ValueError("predict_trim: entry, strand, start and end [K] and seq_off [K + 1] must match")
            up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
            pad = lambda a: a if a.shape[0] else np.zeros(1, a.dtype)
            d = dict(entry=self._dev_u32(pad(np.asarray(clusters["entry"], dtype=np.uint32))),
                     strand=up(pad(np.asarray(clusters["strand"], dtype=np.uint8))),
                     start=self._dev_u32(pad(np.asarray(clusters["start"], dtype=np.uint32))),
                     end=self._dev_u32(pad(np.asarray(clusters["end"], dtype=np.uint32))),
                     seq_off=up(soff.view(np.int64)), seq=up(pad(seq)))
        if min(d[k].numel() for k in ("entry", "strand", "start", "end")) < K or d["seq_off"].numel() < K + 1 or d["seq"].numel() < total:
            raise ValueError("predict_trim: a cluster array is shorter than the %d clusters or %d bytes given" % (K, total))
        cache = repeats.setdefault("_device", {})
        if str(dev) not in cache:
            pad = lambda a: a if a.shape[0] else np.zeros(1, np.uint32)
            cache[str(dev)] = tuple(self._dev_u32(pad(np.ascontiguousarray(repeats[k], dtype=np.uint32))) for k in ("rep_off", "start", "end"))
        r_off, r_start, r_end = cache[str(dev)]
        n_entries, n_elements = int(len(repeats["rep_off"])) - 1, int(len(repeats["start"]))
        e = lambda count, dtype: torch.empty(max(int(count), 1), dtype=dtype, device=dev)
        tmp = self._tmp(self._lib.mrg_predict_trim_temp_bytes, K)
        flag, rep, orig = e(K, torch.uint8), e(K, torch.int32), e(total, torch.uint8)
        kept, kept_off, kept_orig = e(K, torch.int32), e(K + 1, torch.int64), e(total, torch.uint8)
        n_kept, kept_len = C.c_uint64(), C.c_uint64()
        marks = _Marks(timings, dev)
        marks.mark()
        check(self._lib.mrg_predict_trim(self._h, K, d["entry"].data_ptr(), d["strand"].data_ptr(), d["start"].data_ptr(),
                                         d["end"].data_ptr(), d["seq_off"].data_ptr(), d["seq"].data_ptr(), total, n_entries,
                                         r_off.data_ptr(), r_start.data_ptr(), r_end.data_ptr(), n_elements, int(cutoff),
                                         flag.data_ptr(), rep.data_ptr(), orig.data_ptr(), kept.data_ptr(), kept_off.data_ptr(),
                                         kept_orig.data_ptr(), C.byref(n_kept), C.byref(kept_len), tmp.data_ptr(), tmp.numel(),
                                         self._stream_ptr()))
        nk, kl = int(n_kept.value), int(kept_len.value)
        marks.mark()
        out = dict(flag=flag.cpu().numpy()[:K], rep=rep.cpu().numpy()[:K], orig=orig.cpu().numpy()[:total].tobytes(),
                   kept=kept.cpu().numpy()[:nk].view(np.uint32), kept_seq_off=kept_off.cpu().numpy()[:nk + 1].view(np.uint64),
                   kept_orig=kept_orig.cpu().numpy()[:kl].tobytes(),
                   device=dict(flag=flag, rep=rep, orig=orig, kept=kept, kept_seq_off=kept_off, kept_orig=kept_orig, n_kept=nk,
                               kept_len=kl))
        marks.mark()
        if timings is not None:
            timings.update(trim_ms=marks.ms(0, 1), download_ms=marks.ms(1, 2))
        return out

    def predict_trim_reads(self, reads, counts, trim5=1, trim3=3):
        """The reads of a ReadSet that a listing left unaligned, cut for the next one (mrg_predict_trim_reads).  counts: the
        device tensor [4, n] of mrg_list_valid_count (int32 storage).  Returns (sel, ReadSet): sel = the picked reads'
        indices (device, uint32 in int32 storage, read order), the ReadSet = those reads without their first trim5 and last
        trim3 bases (a read of trim5 + trim3 bases or fewer is empty), W as the input's; None in its place when no read is
        picked."""
        torch = _torch()
        n, W, dev = reads.n, reads.W, self.device
        self._expect(counts, torch.int32, "predict_trim_reads: counts")
        if counts.dim() != 2 or int(counts.shape[0]) != 4 or int(counts.shape[1]) < n or (n and int(counts.shape[1]) != n) or \
                not counts.is_contiguous():
            raise ValueError("predict_trim_reads: counts must be a contiguous [4, n] tensor")
        tmp = self._remap_tmp(n, 0)
        sel = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
        o_words = torch.empty(max(W * n, 1), dtype=torch.int64, device=dev)
        o_nmask = None if reads.nmask is None else torch.empty(max(W * n, 1), dtype=torch.int64, device=dev)
        o_lens = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)
        k = C.c_uint64(0)
        check(self._lib.mrg_predict_trim_reads(
            self._h, reads.words.data_ptr(), W, n, reads.lens.data_ptr(), None if reads.nmask is None else reads.nmask.data_ptr(), n,
            counts.data_ptr(), int(trim5), int(trim3), sel.data_ptr(), o_words.data_ptr(), o_lens.data_ptr(),
            None if o_nmask is None else o_nmask.data_ptr(), C.byref(k), tmp.data_ptr(), tmp.numel(), self._stream_ptr()))
        k = int(k.value)
        if k == 0:
            return sel[:0], None
        cut = int(trim5) + int(trim3)
        rs = ReadSet.from_device(o_words[:W * k].view(W, k), o_lens[:k], None if o_nmask is None else o_nmask[:W * k].view(W, k),
                                 None, max(0, reads.min_len - cut), max(0, reads.max_len - cut))
        return sel[:k], rs

    def predict_remap_rows(self, numbers, kept, listing1, listing2, sel):
        """The rows of two listings against the cluster library in the order of the sorted table (mrg_predict_remap_rows).
        numbers [n]: the reads' numbers; kept [K]: the retained clusters (entry j is cluster number kept[j] + 1); listing =
        (offsets int64 [reads + 1], ref int32, pos int32, mm uint8), device tensors, or None for a listing without rows;
        sel [k]: the read of every read of listing2.  Returns device tensors (read, cluster, offset: uint32 in int32 storage;
        mm, pass: uint8), [rows of both]."""
        torch = _torch()
        dev = self.device
        numbers, kept = self._dev_u32(numbers, "predict_remap_rows: numbers"), self._dev_u32(kept, "predict_remap_rows: kept")
        n, K = int(numbers.shape[0]), int(kept.shape[0])

        def listing(ls, reads, what):
            if ls is None:
                return (None, 0, None, None, None)
            off, ref, pos, mm = ls
            self._expect(off, torch.int64, what + " offsets")
            self._expect(ref, torch.int32, what + " ref")
            self._expect(pos, torch.int32, what + " pos")
            self._expect(mm, torch.uint8, what + " mm")
            rows = min(int(ref.shape[0]), int(pos.shape[0]), int(mm.shape[0]))
            if int(off.shape[0]) != reads + 1 or max(int(ref.shape[0]), int(pos.shape[0]), int(mm.shape[0])) != rows:
                raise ValueError("%s: offsets [reads + 1] and ref / pos / mm [rows] must match" % what)
            if rows == 0:
                return (None, 0, None, None, None)
            return (off.contiguous().data_ptr(), rows, ref.contiguous().data_ptr(), pos.contiguous().data_ptr(), mm.contiguous().data_ptr())
        k = 0 if sel is None else int(sel.shape[0])
        if sel is not None:
            sel = self._dev_u32(sel, "predict_remap_rows: sel")
        l1, l2 = listing(listing1, n, "predict_remap_rows: pass 1"), listing(listing2, k, "predict_remap_rows: pass 2")
        T = l1[1] + l2[1]
        tmp = self._remap_tmp(n, T)
        e = lambda dtype: torch.empty(max(T, 1), dtype=dtype, device=dev)
        read, cluster, offset, mm, pass_ = e(torch.int32), e(torch.int32), e(torch.int32), e(torch.uint8), e(torch.uint8)
        check(self._lib.mrg_predict_remap_rows(
            self._h, n, numbers.data_ptr() if n else None, K, kept.data_ptr() if K else None, *l1, k,
            sel.data_ptr() if k else None, *l2, read.data_ptr(), cluster.data_ptr(), offset.data_ptr(), mm.data_ptr(),
            pass_.data_ptr(), tmp.data_ptr(), tmp.numel(), self._stream_ptr()))
        return read[:T], cluster[:T], offset[:T], mm[:T], pass_[:T]

    def predict_remap(self, reads, numbers, lib, kept, seed_len, trims=(1, 3), timings=None):
        """Predict mode's second mapping of a ReadSet against the cluster library `lib` of this engine (reference
        miRge2.0.py:566-601).  Pass 1 lists every read under bowtie's `-n 0 -l seed_len -a --best --norc`; the reads it left
        unaligned are cut by `trims` (`-5 1 -3 3`) and listed under `-n 1 -l 15 -a --best --strata --norc`; the rows of both
        are merged and ordered as `sort -k6,6 -k1,1` orders the table.  numbers [n]: the reads' numbers (device tensor or
        host array); kept [K]: Engine.predict_trim's, host or device.
        Returns a dict: rows = host arrays (read, cluster, offset uint32; mm, pass uint8), n_rows, aligned1 / aligned2 /
        unaligned (reads), and "device" with the rows as device tensors.  timings gets list_ms, rows_ms, download_ms."""
        from .bowtie import N_MODE_MAX_TOTAL
        torch = _torch()
        dev = self.device
        n = reads.n
        marks = _Marks(timings, dev)
        mark = marks.mark
        mark()
        p1 =self._list_valid_device(reads, [lib], 1, STRATUM_ALL, 0, int(seed_len), 0, N_MODE_MAX_TOTAL)
        sel, cut = self.predict_trim_reads(reads, p1["counts"][0], *trims)
        p2 = None
        if cut is not None:
            p2 = self._list_valid_device(cut, [lib], 1, STRATUM_BEST, 0, 15, 1, N_MODE_MAX_TOTAL)

        def listing(p):
            if p is None or p["n_rows"] == 0:
                return None
            return (p["offsets"][0][0], p["ref"][:p["n_rows"]], p["pos"][:p["n_rows"]], p["mm"][:p["n_rows"]])
        mark()
        rows = self.predict_remap_rows(numbers, kept, listing(p1), listing(p2), sel)
        mark()
        host = tuple(t.cpu().numpy().view(np.uint32) if t.dtype == torch.int32 else t.cpu().numpy() for t in rows)
        mark()
        a1 = int(p1["aligned"].sum())
        a2 = 0 if p2 is None else int(p2["aligned"].sum())
        if timings is not None:
            timings.update(list_ms=marks.ms(0, 1), rows_ms=marks.ms(1, 2), download_ms=marks.ms(2, 3))
        return dict(rows=host, n_rows=int(host[0].shape[0]), aligned1=a1, aligned2=a2, unaligned=n - a1 - a2, device=rows)

    def predict_features(self, reads, counts, rows, clusters, entry_len, entry_rank, host_groups=None, timings=None,
                         keep_device=False):
        """Predict mode's cluster feature table from the rows of predict_remap (mrg_predict_feature_groups / _align /
        _tally / _neighbors; the rule of the reference's generate_featureFiles.py and readCluster.py).  reads: the ReadSet
        the rows index; counts [n]: the reads' counts; rows = (read, cluster) device tensors or host arrays in file order;
        clusters: the retained clusters as a dict of entry, strand, start, end, kept [K] (host arrays or device tensors),
        kept_seq_off [K + 1] and kept_orig (bytes); entry_len / entry_rank [entries]: every genome entry's length and the
        position of its name among the sorted names.
        A group with a row the device leaves to the host (a read or cluster beyond 32 nt, an N, a gapped or unsettled
        alignment) is handed to host_groups(g, row_lo, row_hi, cluster) -> None (no stable column) or a dict of H, T, head,
        tail, exact, nine [45]; its numbers join the others before the neighbour step.  Without host_groups such a group
        is an error.
        Returns a dict of host arrays: row_group, row_status, row_diag, row_ident [rows]; group_off [G + 1], group_cluster,
        group_sum, group_pass, group_host, valid, frame [G, 4] (H, T, head, tail), exact, nine [G, 45], nb_t, nb_up, nb_down,
        nb_flags [G]; order [n_sorted] = the groups with a stable column in file order; n_groups, n_passed, n_sorted,
        host_results {g: what host_groups returned}.  timings gets device_ms (events around the four calls, the host groups'
        time included when there are any) and download_ms.
        keep_device=True adds "device" for predict_precursors: the device tensors order, group_cluster, frame, valid, cl_len,
        the clusters' entry, strand, start, end, entry_len, and the ints n_sorted, n_groups, n_clusters."""
        torch = _torch()
        dev = self.device
        n = reads.n
        counts = self._dev_u32(counts, "predict_features: counts")
        row_read, row_cluster = (self._dev_u32(t, "predict_features: rows") for t in rows[:2])
        T = int(row_read.shape[0])
        if int(row_cluster.shape[0]) != T or int(counts.shape[0]) != n:
            raise ValueError("predict_features: rows (read, cluster) must match each other and counts the reads")
        cl = {k: self._dev_u32(clusters[k], "predict_features: " + k) for k in ("entry", "start", "end", "kept")}
        K = int(cl["entry"].shape[0])
        strand = clusters["strand"]
        if not torch.is_tensor(strand):
            strand = torch.from_numpy(np.ascontiguousarray(strand, dtype=np.uint8)).to(dev)
        strand = self._expect(strand, torch.uint8, "predict_features: strand").contiguous()
        soff = np.ascontiguousarray(clusters["kept_seq_off"], dtype=np.uint64)
        orig = np.frombuffer(bytes(clusters["kept_orig"]), dtype=np.uint8)
        if any(int(t.shape[0]) != K for t in (cl["start"], cl["end"], cl["kept"], strand)) or soff.shape != (K + 1,) or \
                int(soff[-1]) != orig.shape[0]:
            raise ValueError("predict_features: entry, strand, start, end, kept [K] and kept_seq_off [K + 1] closing at kept_orig must match")
        entry_len, entry_rank = self._dev_u32(entry_len, "predict_features: entry_len"), self._dev_u32(entry_rank, "predict_features: entry_rank")
        E = int(entry_len.shape[0])
        if int(entry_rank.shape[0]) != E:
            raise ValueError("predict_features: one length and one rank per entry")
        if T and (n == 0 or K == 0 or E == 0):
            raise ValueError("predict_features: rows without reads, clusters or entries")
        d_soff = torch.from_numpy(soff.view(np.int64)).to(dev)
        d_orig = torch.from_numpy(np.array(orig if orig.shape[0] else np.zeros(1, np.uint8))).to(dev)
        e = lambda count, dtype: torch.empty(max(int(count), 1), dtype=dtype, device=dev)
        tmp = self._tmp(self._lib.mrg_predict_feature_temp_bytes, T, floor=64)
        row_group, group_off, group_cluster = e(T, torch.int32), e(T + 1, torch.int32), e(T, torch.int32)
        group_sum, group_pass = e(T, torch.int64), e(T, torch.uint8)
        marks = _Marks(timings, dev)
        mark = marks.mark
        ptr = lambda t: t.data_ptr()
        G, P, S = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        mark()
        check(self._lib.mrg_predict_feature_groups(
            self._h, T, ptr(row_read), ptr(row_cluster), n, ptr(counts), K, ptr(cl["entry"]), ptr(cl["start"]), ptr(cl["end"]),
            ptr(d_soff), int(orig.shape[0]), E, ptr(entry_len), ptr(row_group), ptr(group_off), ptr(group_cluster), ptr(group_sum),
            ptr(group_pass), C.byref(G), C.byref(P), ptr(tmp), tmp.numel(), self._stream_ptr()))
        G = int(G.value)
        cl_word, cl_len = e(K, torch.int64), e(K, torch.uint8)
        row_status, row_diag, row_ident, group_host = e(T, torch.uint8), e(T, torch.int32), e(T, torch.uint8), e(G, torch.uint8)
        check(self._lib.mrg_predict_feature_align(
            self._h, T, ptr(row_read), ptr(row_cluster), ptr(row_group), G, ptr(group_pass), ptr(reads.words) if n else None,
            ptr(reads.lens) if n else None, None if reads.nmask is None else ptr(reads.nmask), n, K, ptr(d_soff), ptr(d_orig),
            int(orig.shape[0]), ptr(cl_word), ptr(cl_len), ptr(row_status), ptr(row_diag), ptr(row_ident), ptr(group_host), ptr(tmp),
            tmp.numel(), self._stream_ptr()))
        valid, frame, exact, nine = e(G, torch.uint8), e(4 * G, torch.int32), e(G, torch.int64), e(45 * G, torch.int64)
        check(self._lib.mrg_predict_feature_tally(
            self._h, G, ptr(group_off), ptr(group_cluster), ptr(group_pass), ptr(group_host), T, ptr(row_read), ptr(row_diag),
            ptr(row_ident), ptr(reads.words) if n else None, ptr(reads.lens) if n else None, n, ptr(counts), K, ptr(cl_len), ptr(valid),
            ptr(frame), ptr(exact), ptr(nine), self._stream_ptr()))
        h_pass, h_host = group_pass.cpu().numpy()[:G], group_host.cpu().numpy()[:G]
        h_off, h_gc = group_off.cpu().numpy()[:G + 1].view(np.uint32), group_cluster.cpu().numpy()[:G].view(np.uint32)
        todo = np.flatnonzero((h_pass != 0) & (h_host != 0))
        host_results = {}
        if todo.size:
            if host_groups is None:
                raise ValueError("predict_features: %d groups hold a row the device leaves to the host and no host_groups was given" % todo.size)
            h_valid, h_frame = valid.cpu().numpy(), frame.cpu().numpy().reshape(-1, 4)
            h_exact, h_nine = exact.cpu().numpy(), nine.cpu().numpy().reshape(-1, 45)
            for g in todo:
                got = host_groups(int(g), int(h_off[g]), int(h_off[g + 1]), int(h_gc[g]))
                host_results[int(g)] = got
                if got is None:
                    continue
                h_valid[g] = 1
                h_frame[g] = (got["H"], got["T"], got["head"], got["tail"])
                h_exact[g] = got["exact"]
                h_nine[g] = got["nine"]
            valid, frame = torch.from_numpy(h_valid).to(dev), torch.from_numpy(h_frame.reshape(-1)).to(dev)
            exact, nine = torch.from_numpy(h_exact).to(dev), torch.from_numpy(h_nine.reshape(-1)).to(dev)
        order, nb_t, nb_flags = e(G, torch.int32), e(G, torch.int32), e(G, torch.uint8)
        nb_up, nb_down = e(G, torch.int64), e(G, torch.int64)
        check(self._lib.mrg_predict_feature_neighbors(
            self._h, G, ptr(group_cluster), ptr(valid), ptr(frame), K, ptr(cl["entry"]), ptr(strand), ptr(cl["start"]), ptr(cl["end"]),
            ptr(cl["kept"]), E, ptr(entry_rank), ptr(order), ptr(nb_t), ptr(nb_up), ptr(nb_down), ptr(nb_flags), C.byref(S), ptr(tmp),
            tmp.numel(), self._stream_ptr()))
        S = int(S.value)
        mark()
        u32 = lambda t, k: t.cpu().numpy()[:k].view(np.uint32)
        out = dict(row_group=u32(row_group, T), row_status=row_status.cpu().numpy()[:T], row_diag=row_diag.cpu().numpy()[:T],
                   row_ident=row_ident.cpu().numpy()[:T], group_off=h_off, group_cluster=h_gc,
                   group_sum=group_sum.cpu().numpy()[:G].view(np.uint64), group_pass=h_pass, group_host=h_host,
                   valid=valid.cpu().numpy()[:G], frame=frame.cpu().numpy()[:4 * G].reshape(G, 4),
                   exact=exact.cpu().numpy()[:G].view(np.uint64), nine=nine.cpu().numpy()[:45 * G].view(np.uint64).reshape(G, 45),
                   nb_t=u32(nb_t, G), nb_up=nb_up.cpu().numpy()[:G], nb_down=nb_down.cpu().numpy()[:G], nb_flags=nb_flags.cpu().numpy()[:G],
                   order=u32(order, G)[:S], n_groups=G, n_passed=int(P.value), n_sorted=S, host_results=host_results)
        mark()
        if keep_device:
            out["device"] = dict(order=order, group_cluster=group_cluster, frame=frame, valid=valid, cl_len=cl_len, entry=cl["entry"],
                                 strand=strand, start=cl["start"], end=cl["end"], entry_len=entry_len, n_sorted=S, n_groups=G,
                                 n_clusters=K)
        if timings is not None:
            timings.update(device_ms=marks.ms(0, 1), download_ms=marks.ms(1, 2))
        return out

    def predict_precursors(self, features_device, clusters=None, entry_len=None, parts_libs=(), timings=None):
        """Predict mode's precursor candidates (mrg_predict_precursors / mrg_predict_precursor_bases; the rule of the
        reference's get_precursors.py): for every group whose line the feature file holds, the two genome windows around the
        stable part of its cluster, as RNA, cut out of the resident genome libraries.  features_device: the "device" dict of
        predict_features(keep_device=True); clusters: a dict of entry, strand, start, end [K] (host arrays or device
        tensors; None: the tensors features_device carries); entry_len [entries] (None: likewise); parts_libs: the keys of
        the genome's parts on this engine, in entry order.
        Returns a dict of host arrays: written (uint8 [n_sorted]), rec_group, rec_lo, rec_hi (uint32 [2 W]), rec_off (uint64
        [2 W + 1]), seq (bytes), n_written = W, and device_ms / download_ms (None without timings, which gets them too)."""
        torch = _torch()
        dev = self.device
        d = features_device
        S, G = int(d["n_sorted"]), int(d["n_groups"])
        order = self._expect(d["order"], torch.int32, "predict_precursors: order")
        group_cluster = self._expect(d["group_cluster"], torch.int32, "predict_precursors: group_cluster")
        frame = self._expect(d["frame"], torch.int32, "predict_precursors: frame")
        valid = self._expect(d["valid"], torch.uint8, "predict_precursors: valid")
        if S > G or order.numel() < S or group_cluster.numel() < G or frame.numel() < 4 * G or valid.numel() < G:
            raise ValueError("predict_precursors: order [n_sorted] and group_cluster, frame [G, 4], valid [G] must hold what the counts say")
        src = d if clusters is None else clusters
        cl = {k: self._dev_u32(src[k], "predict_precursors: " + k) for k in ("entry", "start", "end")}
        strand = src["strand"]
        if not torch.is_tensor(strand):
            strand = torch.from_numpy(np.ascontiguousarray(strand, dtype=np.uint8)).to(dev)
        strand = self._expect(strand, torch.uint8, "predict_precursors: strand").contiguous()
        K = int(d["n_clusters"]) if clusters is None else int(cl["entry"].shape[0])
        if any(int(t.numel()) < K for t in (cl["entry"], cl["start"], cl["end"], strand)):
            raise ValueError("predict_precursors: entry, strand, start and end must hold the K clusters")
        entry_len = self._dev_u32(d["entry_len"] if entry_len is None else entry_len, "predict_precursors: entry_len")
        E = int(entry_len.shape[0])
        lids = np.array([self.libs[k] for k in parts_libs], dtype=np.int32)
        ebase = np.cumsum([0] + [self.indexes[k].n_ref for k in parts_libs]).astype(np.uint32)
        e = lambda count, dtype: torch.empty(max(int(count), 1), dtype=dtype, device=dev)
        tmp = self._tmp(self._lib.mrg_predict_precursor_temp_bytes, S, floor=64)
        written, rec_group, rec_lo, rec_hi = e(S, torch.uint8), e(2 * S, torch.int32), e(2 * S, torch.int32), e(2 * S, torch.int32)
        rec_off = e(2 * S + 1, torch.int64)
        marks = _Marks(timings, dev)
        mark = marks.mark
        ptr = lambda t: t.data_ptr()
        W, total = C.c_uint64(0), C.c_uint64(0)
        mark()
        check(self._lib.mrg_predict_precursors(
            self._h, S, ptr(order), G, ptr(group_cluster), ptr(frame), ptr(valid), K, ptr(cl["entry"]), ptr(strand), ptr(cl["start"]),
            ptr(cl["end"]), E, ptr(entry_len), ptr(written), ptr(rec_group), ptr(rec_lo), ptr(rec_hi), ptr(rec_off), C.byref(W),
            C.byref(total), ptr(tmp), tmp.numel(), self._stream_ptr()))
        W, total = int(W.value), int(total.value)
        seq = e(total, torch.uint8)
        check(self._lib.mrg_predict_precursor_bases(
            self._h, 2 * W, ptr(rec_group), ptr(rec_lo), ptr(rec_hi), ptr(rec_off), G, ptr(group_cluster), K, ptr(cl["entry"]), ptr(strand),
            E, ptr(entry_len), len(lids), lids.ctypes.data if len(lids) else None, ebase.ctypes.data, ptr(seq), total, ptr(tmp),
            tmp.numel(), self._stream_ptr()))
        mark()
        u32 = lambda t, k: t.cpu().numpy()[:k].view(np.uint32)
        out = dict(written=written.cpu().numpy()[:S], rec_group=u32(rec_group, 2 * W), rec_lo=u32(rec_lo, 2 * W), rec_hi=u32(rec_hi, 2 * W),
                   rec_off=rec_off.cpu().numpy()[:2 * W + 1].view(np.uint64), seq=seq.cpu().numpy()[:total].tobytes(), n_written=W,
                   device_ms=None, download_ms=None)
        mark()
        if timings is not None:
            out.update(device_ms=marks.ms(0, 1), download_ms=marks.ms(1, 2))
            timings.update(device_ms=out["device_ms"], download_ms=out["download_ms"])
        return out

    # ---- predict mode: the screening of the folded precursor candidates (csrc/predict_screen.hip)
    def _screen_dev(self, x, np_dtype, torch_dtype, what):
        """A device tensor of torch_dtype as it is; a host array (or bytes) uploaded with np_dtype's bits."""
        torch = _torch()
        if torch.is_tensor(x):
            return self._expect(x, torch_dtype, what).contiguous()
        if isinstance(x, (bytes, bytearray)):
            x = np.frombuffer(bytes(x), dtype=np.uint8)
        a = np.array(x, dtype=np_dtype)   # (a copy: torch wants writable memory)
        signed = {np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}.get(a.dtype)
        if a.size == 0:
            return torch.zeros(1, dtype=torch_dtype, device=self.device)[:0]
        return torch.from_numpy(a.view(signed) if signed else a).to(self.device)

    def _screen_blob(self, off, text, what, text2=None):
        """(offsets tensor, text tensor(s), n, length) of a list of strings given as offsets [n + 1] plus bytes."""
        torch = _torch()
        off = self._screen_dev(off, np.uint64, torch.int64, what + ": offsets")
        if off.numel() < 1:
            raise ValueError("%s: offsets [n + 1] must hold at least the closing one" % what)
        texts = [self._screen_dev(t, np.uint8, torch.uint8, what + ": text") for t in ((text,) if text2 is None else (text, text2))]
        if len(texts) == 2 and texts[0].numel() != texts[1].numel():
            raise ValueError("%s: the sequences' and the structures' bytes must be equally many" % what)
        return off, texts, int(off.numel()) - 1, int(texts[0].numel())

    @staticmethod
    def _p(t):
        return t.data_ptr() if t.numel() else None

    def predict_screen_candidates(self, line_group, nb_flags, nb_up, nb_down):
        """mrg_predict_screen_candidates (screen_precusor_candidates.py:224-285): every feature line's candidate records and
        their miRNAs.  line_group [n_lines]; nb_flags, nb_up, nb_down [n_groups] as Engine.predict_features leaves them (host
        arrays or device tensors).  Returns device tensors cand_n [n_lines], cand_rec [4 n_lines] and cand_mir [8 n_lines]
        (-1 = unused slot / no second miRNA).  MirgeAmdError naming the line where the reference dies."""
        torch = _torch()
        lg = self._dev_u32(line_group, "predict_screen_candidates: line_group")
        flags = self._screen_dev(nb_flags, np.uint8, torch.uint8, "predict_screen_candidates: nb_flags")
        up = self._screen_dev(nb_up, np.int64, torch.int64, "predict_screen_candidates: nb_up")
        down = self._screen_dev(nb_down, np.int64, torch.int64, "predict_screen_candidates: nb_down")
        n, G = int(lg.numel()), int(flags.numel())
        if up.numel() != G or down.numel() != G:
            raise ValueError("predict_screen_candidates: nb_flags, nb_up and nb_down must hold one entry a group")
        e = lambda count, dtype: torch.empty(max(int(count), 1), dtype=dtype, device=self.device)[:int(count)]
        cand_n, cand_rec, cand_mir = e(n, torch.uint8), e(4 * n, torch.int32), e(8 * n, torch.int32)
        tmp = self._screen_tmp(0)
        p = self._p
        check(self._lib.mrg_predict_screen_candidates(self._h, n, p(lg), G, p(flags), p(up), p(down), p(cand_n), p(cand_rec), p(cand_mir),
                                                      tmp.data_ptr(), tmp.numel(), self._stream_ptr()))
        return dict(cand_n=cand_n, cand_rec=cand_rec, cand_mir=cand_mir)

    def predict_screen_prune(self, cand_rec, cand_mir, rec_off, seq, structure, mir_off, mir, pruned_length=15):
        """mrg_predict_screen_prune: getPrunedPrecusor up to its fold.  cand_rec [n_cand] / cand_mir [2 n_cand] as
        predict_screen_candidates returns them; records and miRNAs as offsets [n + 1] plus bytes.  Returns host arrays: status
        (0 None, 1 cut, 2 left to the host, 3 unused slot), lo, hi (the slice of the record), pruned_off [n_cand + 1], pruned."""
        torch = _torch()
        rec = self._dev_u32(cand_rec, "predict_screen_prune: cand_rec")
        cm = self._dev_u32(cand_mir, "predict_screen_prune: cand_mir")
        n = int(rec.numel())
        if cm.numel() != 2 * n:
            raise ValueError("predict_screen_prune: cand_mir must hold two entries a candidate")
        roff, (d_seq, d_str), n_rec, seq_len = self._screen_blob(rec_off, seq, "predict_screen_prune: records", structure)
        moff, (d_mir,), n_mir, mir_len = self._screen_blob(mir_off, mir, "predict_screen_prune: miRNAs")
        e = lambda count, dtype: torch.empty(max(int(count), 1), dtype=dtype, device=self.device)[:int(count)]
        status, lo, hi, poff = e(n, torch.uint8), e(n, torch.int32), e(n, torch.int32), e(n + 1, torch.int64)
        cap = n * 256   # (a slice the kernel cuts comes from a record of at most 256 characters)
        pruned = e(cap, torch.uint8)
        tmp = self._screen_tmp(n)
        total = C.c_uint64(0)
        p = self._p
        check(self._lib.mrg_predict_screen_prune(
            self._h, n, p(rec), p(cm), n_rec, p(roff), p(d_seq), p(d_str), seq_len, n_mir, p(moff), p(d_mir), mir_len, int(pruned_length),
            p(status), p(lo), p(hi), p(poff), p(pruned), cap, C.byref(total), tmp.data_ptr(), tmp.numel(), self._stream_ptr()))
        u32 = lambda t: t.cpu().numpy().view(np.uint32)
        return dict(status=status.cpu().numpy(), lo=u32(lo), hi=u32(hi), pruned_off=poff.cpu().numpy().view(np.uint64),
                    pruned=pruned[:int(total.value)].cpu().numpy().tobytes())

    def predict_screen_features(self, status, cand_mir, p_off, p_seq, p_str, mir_off, mir):
        """mrg_predict_screen_features: featuresInPrecusor and its two companions for every candidate with status 1, from its
        pruned sequence and new structure (p_off [n_cand + 1], p_seq, p_str).  Returns int32 [n_cand, 16] on the host
        (include/mirge_amd.h names the words; word 0 = 2: left to the host)."""
        torch = _torch()
        st = self._screen_dev(status, np.uint8, torch.uint8, "predict_screen_features: status")
        cm = self._dev_u32(cand_mir, "predict_screen_features: cand_mir")
        n = int(st.numel())
        poff, (d_seq, d_str), n_p, p_len = self._screen_blob(p_off, p_seq, "predict_screen_features: pruned", p_str)
        moff, (d_mir,), n_mir, mir_len = self._screen_blob(mir_off, mir, "predict_screen_features: miRNAs")
        if cm.numel() != 2 * n or n_p != n:
            raise ValueError("predict_screen_features: status [n], cand_mir [2 n] and p_off [n + 1] must match")
        feat = torch.empty(max(16 * n, 1), dtype=torch.int32, device=self.device)[:16 * n]
        tmp = self._screen_tmp(n)
        p = self._p
        check(self._lib.mrg_predict_screen_features(self._h, n, p(st), p(cm), p(poff), p(d_seq), p(d_str), p_len, n_mir, p(moff), p(d_mir),
                                                    mir_len, p(feat), tmp.data_ptr(), tmp.numel(), self._stream_ptr()))
        return feat.cpu().numpy().reshape(n, 16)

    def predict_screen_select(self, cand_n, cand_rec, rec_mfe, feat, threshold=15):
        """mrg_predict_screen_select: selcteOptimalPrecusor per line over feat [4 n_lines, 16] (the host's rows filled in) by
        the records' original energies rec_mfe [2 n_lines].  Returns best (int32 [n_lines], -1 = None) on the host."""
        torch = _torch()
        cn = self._screen_dev(cand_n, np.uint8, torch.uint8, "predict_screen_select: cand_n")
        rec = self._dev_u32(cand_rec, "predict_screen_select: cand_rec")
        mfe = self._screen_dev(rec_mfe, np.float64, torch.float64, "predict_screen_select: rec_mfe")
        ft = self._screen_dev(np.asarray(feat).reshape(-1) if not torch.is_tensor(feat) else feat.reshape(-1), np.int32, torch.int32,
                              "predict_screen_select: feat")
        n = int(cn.numel())
        if rec.numel() != 4 * n or ft.numel() != 64 * n:
            raise ValueError("predict_screen_select: cand_n [n], cand_rec [4 n] and feat [4 n, 16] must match")
        best = torch.empty(max(n, 1), dtype=torch.int32, device=self.device)[:n]
        tmp = self._screen_tmp(0)
        p = self._p
        check(self._lib.mrg_predict_screen_select(self._h, n, p(cn), p(rec), int(mfe.numel()), p(mfe), p(ft), int(threshold), p(best),
                                                  tmp.data_ptr(), tmp.numel(), self._stream_ptr()))
        return best.cpu().numpy()

    # ---- predict mode: the SVM of the model file (csrc/predict_svm.hip)
    def predict_svm(self, x, model):
        """mrg_predict_svm: sklearn's predict, decision_function and predict_proba of the model file's scaler and SVC for raw
        feature rows x [n, nf] (float64; a host array or a device tensor).  model: svm_model.SvmModel.  Returns host arrays:
        pred (int8 [n], 1 or -1), dec (float64 [n]) and prob (float64 [n, 2]: class -1, class 1)."""
        torch = _torch()
        nf, n_sv = int(model.sv.shape[1]), int(model.sv.shape[0])
        xd = self._screen_dev(x.reshape(-1) if torch.is_tensor(x) else np.asarray(x, dtype=np.float64).reshape(-1), np.float64,
                              torch.float64, "predict_svm: x")
        if xd.numel() % nf:
            raise ValueError("predict_svm: x must hold rows of the model's %d features" % nf)
        if model.mean.shape != (nf,) or model.scale.shape != (nf,) or model.coef.shape != (n_sv,):
            raise ValueError("predict_svm: the model's mean and scale [nf], sv [n_sv, nf] and coef [n_sv] must match")
        n = int(xd.numel()) // nf
        up = lambda a, what: self._screen_dev(np.asarray(a).reshape(-1), np.float64, torch.float64, "predict_svm: " + what)
        mean, scale, sv, coef = up(model.mean, "mean"), up(model.scale, "scale"), up(model.sv, "sv"), up(model.coef, "coef")
        e = lambda count, dtype: torch.empty(max(int(count), 1), dtype=dtype, device=self.device)[:int(count)]
        pred, dec, prob = e(n, torch.int8), e(n, torch.float64), e(2 * n, torch.float64)
        p = self._p
        check(self._lib.mrg_predict_svm(self._h, n, p(xd), nf, p(mean), p(scale), p(sv), p(coef), n_sv, float(model.intercept),
                                        float(model.gamma), float(model.probA), float(model.probB), p(pred), p(dec), p(prob),
                                        self._stream_ptr()))
        return dict(pred=pred.cpu().numpy(), dec=dec.cpu().numpy(), prob=prob.cpu().numpy().reshape(n, 2))

    # ---- predict mode: the report (csrc/predict_report.hip)
    _REPORT_LINE_ARRAYS = (("flags", np.uint8, "uint8"), ("rank", np.uint32, "int32"), ("up", np.int64, "int64"), ("down", np.int64, "int64"),
                           ("pos", np.int64, "int64"), ("adj", np.int32, "int32"), ("reads", np.int64, "int64"), ("gid3", np.uint32, "int32"),
                           ("t_off", np.uint64, "int64"), ("text", np.uint8, "uint8"), ("blk", np.uint8, "uint8"), ("r_off", np.uint64, "int64"),
                           ("row_start", np.int64, "int64"), ("row_end", np.int64, "int64"), ("row_count", np.int64, "int64"),
                           ("row_soff", np.uint64, "int64"), ("row_text", np.uint8, "uint8"))

    def _report_tmp(self, n):
        return self._tmp(self._lib.mrg_predict_report_temp_bytes, n, floor=64)

    def predict_report_upload(self, arrays):
        """The native reader's arrays (predict.ReportInputs.arrays, or tests/predict_report_model.arrays) as device tensors."""
        torch = _torch()
        d = {k: self._screen_dev(np.asarray(arrays[k]).reshape(-1) if not isinstance(arrays[k], (bytes, bytearray)) else arrays[k], np_dt,
                                 getattr(torch, t_dt), "predict_report: " + k) for k, np_dt, t_dt in self._REPORT_LINE_ARRAYS}
        n = int(d["flags"].numel())
        sizes = dict(rank=n, up=n, down=n, pos=2 * n, adj=4 * n, reads=n, gid3=3 * n, t_off=4 * n + 1, blk=n, r_off=n + 1)
        R = int(d["row_start"].numel())
        sizes.update(row_end=R, row_count=R, row_soff=R + 1)
        for k, want in sizes.items():
            if int(d[k].numel()) != want:
                raise ValueError("predict_report: %s must hold %d entries, not %d" % (k, want, int(d[k].numel())))
        d["n"], d["n_rows"] = n, R
        return d

    def predict_report_correct(self, d):
        """mrg_predict_report_correct over predict_report_upload's tensors: device tensors src, state, err, pos_adj, stable_idx, gid."""
        torch = _torch()
        n = d["n"]
        e = lambda count, dtype: torch.empty(max(int(count), 1), dtype=dtype, device=self.device)[:int(count)]
        out = dict(src=e(n, torch.int32), state=e(n, torch.uint8), err=e(n, torch.uint8), pos_adj=e(2 * n, torch.int64),
                   stable_idx=e(n, torch.int32), gid=e(n, torch.int32))
        p = self._p
        check(self._lib.mrg_predict_report_correct(self._h, n, p(d["flags"]), p(d["up"]), p(d["down"]), p(d["pos"]), p(d["adj"]), p(d["gid3"]),
                                                   p(d["t_off"]), p(d["text"]), int(d["text"].numel()), p(out["src"]), p(out["state"]),
                                                   p(out["err"]), p(out["pos_adj"]), p(out["stable_idx"]), p(out["gid"]), self._stream_ptr()))
        return out

    def predict_report_entries(self, d, lines):
        """mrg_predict_report_entries: device tensors ent_m, ent_p, chunk_err, chunk_line [n], row_off, prof_off [n + 1] and the
        totals n_entries, rows, words."""
        torch = _torch()
        n = d["n"]
        e = lambda count, dtype: torch.empty(max(int(count), 1), dtype=dtype, device=self.device)[:int(count)]
        out = dict(ent_m=e(n, torch.int32), ent_p=e(n, torch.int32), chunk_err=e(n, torch.uint8), chunk_line=e(n, torch.int32),
                   row_off=e(n + 1, torch.int64), prof_off=e(n + 1, torch.int64))
        totals = (C.c_uint64 * 3)()
        tmp = self._report_tmp(n)
        p = self._p
        check(self._lib.mrg_predict_report_entries(self._h, n, p(d["flags"]), p(d["rank"]), p(d["reads"]), p(d["t_off"]), p(lines["src"]),
                                                   p(lines["state"]), p(lines["stable_idx"]), p(lines["gid"]), p(d["blk"]), p(d["r_off"]),
                                                   p(out["ent_m"]), p(out["ent_p"]), p(out["chunk_err"]), p(out["chunk_line"]),
                                                   p(out["row_off"]), p(out["prof_off"]), totals, tmp.data_ptr(), tmp.numel(),
                                                   self._stream_ptr()))
        out.update(n_entries=int(totals[0]), rows=int(totals[1]), words=int(totals[2]))
        return out

    def predict_report_profile(self, d, lines, ents):
        """mrg_predict_report_profile: device tensors lead, trail [rows], prof [words], total, flag [n_entries]."""
        torch = _torch()
        n, E = d["n"], ents["n_entries"]
        e = lambda count, dtype: torch.zeros(max(int(count), 1), dtype=dtype, device=self.device)[:int(count)]
        out = dict(lead=e(ents["rows"], torch.int32), trail=e(ents["rows"], torch.int32), prof=e(ents["words"], torch.int64),
                   total=e(E, torch.int64), flag=e(E, torch.uint8))
        p = self._p
        check(self._lib.mrg_predict_report_profile(self._h, n, p(d["flags"]), p(d["t_off"]), p(d["text"]), int(d["text"].numel()),
                                                   p(lines["src"]), p(lines["pos_adj"]), p(lines["stable_idx"]), p(d["r_off"]), d["n_rows"],
                                                   p(d["row_start"]), p(d["row_end"]), p(d["row_count"]), p(d["row_soff"]), p(d["row_text"]),
                                                   int(d["row_text"].numel()), E, p(ents["ent_m"]), p(ents["ent_p"]), p(ents["row_off"]),
                                                   p(ents["prof_off"]), p(out["lead"]), p(out["trail"]), p(out["prof"]), p(out["total"]),
                                                   p(out["flag"]), self._stream_ptr()))
        return out

    REPORT_ERRORS = {1: "upstreamDistance is no whole number", 2: "upstreamDistance exceeds 44 and downstreamDistance is None or no whole number",
                     3: "the last line offers its precursor to a line that does not exist",
                     4: "the name is in the novel list and its precursor is None",
                     5: "the line is the mature one of its pair, is not loop and is not in the novel list",
                     6: "a stable sequence of its pair is not in the precursor", 7: "the cluster file holds no (or a malformed) block of its pair",
                     8: "offsets that do not ascend inside their text"}

    def predict_report(self, arrays, host_line=None, host_entry=None, timings=None):
        """The report's three device calls over the native reader's arrays (mrg_predict_report_correct / _entries / _profile).
        host_line(j, src) -> (re-typed, stable index) answers for the lines the correction leaves to the host (state & 4), and
        host_entry(e, m, p, src, pos_adj, stable_idx) -> (lead, trail, sums, total, ragged) for the entries the profile leaves
        (flag & 2); without them such a line or entry is an error.  Returns host arrays: src, state, pos_adj, stable_idx, gid,
        ent_m, ent_p, row_off, prof_off, lead, trail, prof, total, flag, and n_entries, host_lines, host_entries.  ValueError
        naming the line and the reason where the reference raises."""
        torch = _torch()
        d = self.predict_report_upload(arrays)
        n = d["n"]
        lines = self.predict_report_correct(d)

        def refuse(code, line):
            raise ValueError("line %d of the table: %s" % (int(line) + 2, self.REPORT_ERRORS.get(int(code), "error %d" % int(code))))
        err = lines["err"].cpu().numpy()
        if err.any():
            j = int(np.flatnonzero(err)[0])
            refuse(err[j], j)
        state = lines["state"].cpu().numpy()
        src = lines["src"].cpu().numpy().view(np.uint32)
        left = np.flatnonzero(state & 4)
        if left.size:
            if host_line is None:
                raise ValueError("line %d of the table: a precursor beyond 256 or a sequence beyond 255 characters" % (int(left[0]) + 2))
            stable = lines["stable_idx"].cpu().numpy()
            for j in left.tolist():
                retyped, at = host_line(j, int(src[j]))
                arm = (int(state[j]) >> 4) & 3
                if retyped and arm != 2:
                    state[j] = (int(state[j]) & 0x0f) | 2 | (2 << 4)
                stable[j] = at
            lines["state"] = torch.from_numpy(state).to(self.device)
            lines["stable_idx"] = torch.from_numpy(stable).to(self.device)
        ents = self.predict_report_entries(d, lines)
        cerr = ents["chunk_err"].cpu().numpy()
        if cerr.any():
            k = int(np.flatnonzero(cerr)[0])
            refuse(cerr[k], ents["chunk_line"].cpu().numpy().view(np.uint32)[k])
        E = ents["n_entries"]
        prof = self.predict_report_profile(d, lines, ents)
        u32 = lambda t: t.cpu().numpy().view(np.uint32)
        u64 = lambda t: t.cpu().numpy().view(np.uint64)
        out = dict(src=src, state=state, pos_adj=lines["pos_adj"].cpu().numpy().reshape(n, 2), stable_idx=lines["stable_idx"].cpu().numpy(),
                   gid=u32(lines["gid"]), ent_m=u32(ents["ent_m"])[:E].copy(), ent_p=ents["ent_p"].cpu().numpy()[:E].copy(),
                   row_off=u64(ents["row_off"])[:E + 1].copy(), prof_off=u64(ents["prof_off"])[:E + 1].copy(), lead=prof["lead"].cpu().numpy(),
                   trail=prof["trail"].cpu().numpy(), prof=u64(prof["prof"]), total=u64(prof["total"]), flag=prof["flag"].cpu().numpy(),
                   n_entries=E, host_lines=int(left.size))
        if E == 0:
            out["row_off"], out["prof_off"] = np.zeros(1, np.uint64), np.zeros(1, np.uint64)
        if (out["flag"] & 4).any():
            raise _native.MirgeAmdError(-1, "predict_report: entry %d: arrays that contradict each other" % (int(np.flatnonzero(out["flag"] & 4)[0]) + 1))
        left_e = np.flatnonzero(out["flag"] & 2)
        out["host_entries"] = int(left_e.size)
        for e in left_e.tolist():
            if host_entry is None:
                raise ValueError("entry %d: a precursor beyond 256, a read beyond 255 characters or more than 65535 dashes" % (e + 1))
            lead, trail, sums, total, ragged = host_entry(e, int(out["ent_m"][e]), int(out["ent_p"][e]), src, out["pos_adj"], out["stable_idx"])
            r0, r1, p0, p1 = int(out["row_off"][e]), int(out["row_off"][e + 1]), int(out["prof_off"][e]), int(out["prof_off"][e + 1])
            out["lead"][r0:r1], out["trail"][r0:r1], out["prof"][p0:p1] = lead, trail, sums
            out["total"][e], out["flag"][e] = total, 1 if ragged else 0
        return out

    def trf_peaks(self, off, codes, nmask, span, rpm, max_len, ktab):
        """Density peaks of `-trf` (W2C:417-533, :951-961) for every (sample, tRNA) group of a run, through
        mrg_trf_rho / _delta / _border.  Host arrays: off[G+1] row offsets, codes / nmask [W][n] uint64 (nmask
        None without N), span[n] uint16 (first | last << 8), rpm[n] float64, ktab = K[d] (float64, d < len).
        Runs the rho pass now and returns a TrfPeaks: .rho (float32[n]) and .max_dis (uint32[G]) on the host,
        .min_distance(rank) and .border(labels, bord_off) for the two later passes."""
        torch = _torch()
        off = np.ascontiguousarray(off, dtype=np.uint32)
        G, n = len(off) - 1, int(off[-1])
        signed = {np.dtype(np.uint64): np.int64, np.dtype(np.uint16): np.int16}  # (same bits; torch copies them)
        dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt).view(signed.get(np.dtype(dt), dt))).to(self.device)
        t = TrfPeaks(self, off, max_len)
        t.codes = dev(np.asarray(codes).reshape(-1) if n else np.zeros(1), np.uint64)
        t.nmask = dev(np.asarray(nmask).reshape(-1), np.uint64) if nmask is not None and n else None
        t.span = dev(span if n else np.zeros(1), np.uint16)
        rpm_d = dev(rpm if n else np.zeros(1), np.float64)
        return self._trf_rho(t, rpm_d, ktab)

    def trf_peaks_groups(self, groups, ktab):
        """Engine.trf_peaks on the device tensors of a TrfGroups (Engine.trf_sample_groups): no host layout, no upload."""
        t = TrfPeaks(self, np.ascontiguousarray(groups.off, dtype=np.uint32), groups.max_len)
        t.codes, t.nmask, t.span = groups.codes_d, groups.nmask_d, groups.span_d
        t.counts_d = None if groups.rows_d is None else groups.rows_d[:, 1]
        return self._trf_rho(t, groups.rpm_d, ktab)

    def _trf_rho(self, t, rpm_d, ktab):
        torch = _torch()
        G, n, max_len = t.G, t.n, t.max_len
        kt = np.ascontiguousarray(ktab, dtype=np.float64)
        rho = torch.empty(max(n, 1), dtype=torch.float32, device=self.device)
        t.max_dis_d = torch.empty(max(G, 1), dtype=torch.int32, device=self.device)
        check(self._lib.mrg_trf_rho(self._h, t.off_c, G, int(max_len), t.codes.data_ptr(), t.nmask_ptr(),
                                    t.span.data_ptr(), rpm_d.data_ptr(),
                                    kt.ctypes.data_as(C.POINTER(C.c_double)), len(kt), rho.data_ptr(),
                                    t.max_dis_d.data_ptr(), self._stream_ptr()))
        t.rho_d = rho
        t.rho = rho.cpu().numpy()[:n]
        t.max_dis = t.max_dis_d.cpu().numpy()[:G].view(np.uint32)
        return t

    # ------------------------------------------------------------------
    def annotate_host(self, words, lens, nmask, passes, quant=None, n_mirna=0,
                      canon_pass=CANON_PASS, isomir_pass=ISOMIR_PASS):
        """Host-buffer path of the C-ABI (mrg_annotate_host): numpy in, numpy out."""
        words = np.ascontiguousarray(words, dtype=np.uint64)
        W, n = words.shape
        lens = np.ascontiguousarray(lens, dtype=np.uint8)
        nm = None if nmask is None else np.ascontiguousarray(nmask, dtype=np.uint64)
        n_pass = len(passes)
        pass_id = np.empty(n, dtype=np.int8)
        ref_id = np.empty(n, dtype=np.int32)
        pos = np.empty(n, dtype=np.int32)
        mm = np.empty(n, dtype=np.uint8)
        st = (PassStats * n_pass)()
        counts = None
        q = None
        S = 0
        if quant is not None:
            q = np.ascontiguousarray(quant, dtype=np.uint32)
            if q.ndim == 1:
                q = q[:, None]
            S = q.shape[1]
            counts = np.zeros(self.counts_len(n_mirna, S, n_pass), dtype=np.uint64)
        check(self._lib.mrg_annotate_host(
            self._h, words.ctypes.data, W, lens.ctypes.data, None if nm is None else nm.ctypes.data,
            n, passes, n_pass, pass_id.ctypes.data, ref_id.ctypes.data, pos.ctypes.data,
            mm.ctypes.data, st, None if q is None else q.ctypes.data, S, n_mirna, canon_pass,
            isomir_pass, None if counts is None else counts.ctypes.data))
        stats = [dict(processed=int(s.processed), aligned=int(s.aligned), steps=int(s.steps),
                      candidates=int(s.candidates), lookups=int(s.lookups), ms=float(s.ms),
                     lds_bytes=int(s.lds_bytes), lds_mode=int(s.lds_mode), group=int(s.group),
                      n_launches=int(s.n_launches), kbits_log2=int(s.kbits_log2),
                     pair_anchor=int(s.pair_anchor), ms_rest=float(s.ms_rest), variant=int(s.variant))
                 for s in st]
        return dict(pass_id=pass_id, ref_id=ref_id, pos=pos, mm=mm, stats=stats, counts=counts)


PACKED_REF_SAT, PACKED_POS_SAT = 0x3FFFF, 0xFF


class TrfGroups:
    """Result of Engine.trf_sample_groups.  Host: n_items, blocks int32 [B, 6] (sample, representative entry, first and
    number of printed rows, group or -1, 0), block_sums uint64 [B], off uint32 [G + 1], groups int32 [G, 2] (its block, the
    block whose name it is paired with), rows uint32 [n, 3] (tsv row, count, type), max_len, has_n, no_template_row.
    Device: codes_d / nmask_d (None without N) [W][n], span_d, rpm_d, rows_d; .codes / .nmask / .span / .rpm download them."""
    codes_d = nmask_d = span_d = rpm_d = rows_d = None
    rows = np.zeros((0, 3), dtype=np.uint32)

    def _host(self, t, view, shape):
        return t.cpu().numpy().view(view).reshape(shape)

    @property
    def codes(self):
        W = (self.max_len + 31) // 32
        return self._host(self.codes_d, np.uint64, (W, -1))[:, :self.n]

    @property
    def nmask(self):
        W = (self.max_len + 31) // 32
        return None if self.nmask_d is None else self._host(self.nmask_d, np.uint64, (W, -1))[:, :self.n]

    @property
    def span(self):
        return self._host(self.span_d, np.uint16, (-1,))[:self.n]

    @property
    def rpm(self):
        return self._host(self.rpm_d, np.float64, (-1,))[:self.n]


class TrfPeaks:
    """Device state of one Engine.trf_peaks batch (see there)."""
    rank_d = delta_d = nneigh_d = label_d = bord_d = counts_d = None

    def __init__(self, engine, off, max_len):
        self.engine, self.off, self.max_len = engine, off, int(max_len)
        self.off_c = off.ctypes.data_as(C.POINTER(C.c_uint32))
        self.G, self.n = len(off) - 1, int(off[-1])

    def nmask_ptr(self):
        return self.nmask.data_ptr() if self.nmask is not None else None

    def rank(self):
        """Each group's rows (group-local) in rank order -- the stable sort of -rho -- flat like the rows (mrg_trf_rank).
        Stays on the device for min_distance(None); returned as uint32[n]."""
        torch = _torch()
        e = self.engine
        self.rank_d = torch.zeros(max(self.n, 1), dtype=torch.int32, device=e.device)
        if self.G:
            check(e._lib.mrg_trf_rank(e._h, self.off_c, self.G, self.rho_d.data_ptr(), self.rank_d.data_ptr(), e._stream_ptr()))
        return self.rank_d.cpu().numpy()[:self.n].view(np.uint32)

    def min_distance(self, rank=None):
        """min_distance (W2C:509-533): rank = each group's rows (group-local) in rank order, flat like the rows (None:
        what rank() left on the device).  Returns (delta, nneigh) int32[n]: distance to / group-local row of the nearest
        row ranked above, -1 for the top row of a group.  Both stay on the device for assign()."""
        torch = _torch()
        e = self.engine
        if rank is None:
            if self.rank_d is None:
                raise ValueError("min_distance(None) needs rank() first")
            rank_d = self.rank_d
        else:
            rank_d = torch.from_numpy(np.ascontiguousarray(rank if self.n else np.zeros(1), dtype=np.uint32)
                                      .view(np.int32)).to(e.device)
        delta = torch.empty(max(self.n, 1), dtype=torch.int32, device=e.device)
        nneigh = torch.empty(max(self.n, 1), dtype=torch.int32, device=e.device)
        check(e._lib.mrg_trf_delta(e._h, self.off_c, self.G, self.max_len, self.codes.data_ptr(), self.nmask_ptr(),
                                   self.span.data_ptr(), rank_d.data_ptr(), self.max_dis_d.data_ptr(),
                                   delta.data_ptr(), nneigh.data_ptr(), e._stream_ptr()))
        self.delta_d, self.nneigh_d = delta, nneigh
        return delta.cpu().numpy()[:self.n], nneigh.cpu().numpy()[:self.n]

    def assign(self):
        """Cluster centres and labels (mrg_trf_assign) from what rank() and min_distance() left on the device.  Returns
        (nclust uint32[G], cen_off uint32[G + 1], centers uint32[cen_off[-1]]: the group-local row of every centre, cluster 1
        first); the labels (int32[n], -1 or 1..NCLUST) stay on the device for border(None, ...) and halo(); .labels()
        downloads them."""
        torch = _torch()
        e = self.engine
        if self.rank_d is None or self.delta_d is None:
            raise ValueError("assign() needs rank() and min_distance() first")
        nclust, cen_off = np.zeros(self.G, dtype=np.uint32), np.zeros(self.G + 1, dtype=np.uint32)
        centers = np.zeros(max(self.n, 1), dtype=np.uint32)
        label = torch.zeros(max(self.n, 1), dtype=torch.int32, device=e.device)
        if self.G:
            check(e._lib.mrg_trf_assign(e._h, self.off_c, self.G, self.rho_d.data_ptr(), self.rank_d.data_ptr(),
                                        self.delta_d.data_ptr(), self.nneigh_d.data_ptr(), label.data_ptr(), nclust.ctypes.data,
                                        self.n, cen_off.ctypes.data, centers.ctypes.data, e._stream_ptr()))
        self.label_d, self.cen_off, self.centers = label, cen_off, centers[:int(cen_off[-1])]
        return nclust, cen_off, self.centers

    def labels(self):
        return self.label_d.cpu().numpy()[:self.n]

    def border(self, labels, bord_off):
        """Border densities (W2C:951-961): labels int32[n] (-1 or 1..NCLUST; None: what assign() left on the device),
        bord_off[G+1] (NCLUST + 1 slots per group, none where NCLUST <= 1).  Returns float32[bord_off[-1]]."""
        torch = _torch()
        e = self.engine
        bo = np.ascontiguousarray(bord_off, dtype=np.uint32)
        nb = int(bo[-1])
        if labels is None:
            if self.label_d is None:
                raise ValueError("border(None, ...) needs assign() first")
            lab = self.label_d
        else:
            lab = torch.from_numpy(np.ascontiguousarray(labels if self.n else np.zeros(1), dtype=np.int32)).to(e.device)
        bord = torch.empty(max(nb, 1), dtype=torch.float32, device=e.device)
        check(e._lib.mrg_trf_border(e._h, self.off_c, self.G, self.max_len, self.codes.data_ptr(), self.nmask_ptr(),
                                    self.span.data_ptr(), self.rho_d.data_ptr(), lab.data_ptr(),
                                    bo.ctypes.data_as(C.POINTER(C.c_uint32)), bord.data_ptr(), e._stream_ptr()))
        self.bord_d, self.bord_off = bord, bo
        return bord.cpu().numpy()[:nb]

    def halo(self, counts=None):
        """Core / halo of every row and the tallies of every cluster (mrg_trf_halo), after assign() and border(None, ...).
        counts: the read count of every row (uint32[n]; None: the rows that Engine.trf_sample_groups left on the device).
        Returns (core uint8[n], order uint32[n]: the rows by (group, cluster; label -1 last), a cluster's members in row
        order; tallies uint64[cen_off[-1], 4]: members, core rows, read count in the core, read count in the halo)."""
        torch = _torch()
        e = self.engine
        if self.label_d is None or self.bord_d is None:
            raise ValueError("halo() needs assign() and border() first")
        if counts is None:
            if self.counts_d is None:
                raise ValueError("halo() needs the read counts of the rows")
            cnt = self.counts_d
        else:
            cnt = torch.from_numpy(np.ascontiguousarray(counts if self.n else np.zeros(1), dtype=np.uint32).view(np.int32)).to(e.device)
        core = torch.zeros(max(self.n, 1), dtype=torch.uint8, device=e.device)
        order = torch.zeros(max(self.n, 1), dtype=torch.int32, device=e.device)
        tallies = np.zeros((len(self.centers), 4), dtype=np.uint64)
        if self.G:
            check(e._lib.mrg_trf_halo(e._h, self.off_c, self.G, self.max_len, self.codes.data_ptr(), self.nmask_ptr(),
                                      self.span.data_ptr(), self.rho_d.data_ptr(), self.label_d.data_ptr(), cnt.data_ptr(),
                                      int(cnt.stride(0)), self.cen_off.ctypes.data, self.centers.ctypes.data,
                                      self.bord_off.ctypes.data, self.bord_d.data_ptr(), core.data_ptr(), order.data_ptr(),
                                      tallies.ctypes.data, e._stream_ptr()))
        return core.cpu().numpy()[:self.n], order.cpu().numpy()[:self.n].view(np.uint32), tallies


def unpack_assignments(packed):
    """Host side of Engine.pack_assignments: (pass_id int8, ref_id int32, pos int32, mm uint8) from the
    packed words (numpy); ref_id == PACKED_REF_SAT / pos == PACKED_POS_SAT / mm == 3 mean "at least"."""
    w = np.asarray(packed).view(np.uint32)
    code = (w >> 28).astype(np.int16)
    pass_id = (code - 1).astype(np.int8)
    none = code == 0
    ref = ((w >> 8) & 0x3FFFF).astype(np.int32)
    pos = (w & 0xFF).astype(np.int32)
    mm = ((w >> 26) & 3).astype(np.uint8)
    ref[none] = -1
    pos[none] = -1
    mm[none] = 0
    return pass_id, ref, pos, mm


def split_counts(counts, n_mirna, n_samples, n_pass):
    """Views into the fused count vector (layout of mrg_tally_run)."""
    M, S = n_mirna, n_samples
    c = np.asarray(counts).astype(np.int64)
    quant = c[:M * S].reshape(M, S)
    iscan = c[M * S:2 * M * S].reshape(M, S)
    cat = c[2 * M * S:2 * M * S + (n_pass + 1) * S].reshape(n_pass + 1, S)
    uniq = c[2 * M * S + (n_pass + 1) * S:2 * M * S + (n_pass + 2) * S]
    return quant, iscan, cat, uniq


def split_edit_counts(counts, n_bins, n_samples):
    """Views into the vector of mrg_edit_tally_run: (totals [bins, S, 3] = count_true, seq_true,
    canonical; positions [bins, 32, S])."""
    c = np.asarray(counts).astype(np.int64)
    k = n_bins * n_samples * 3
    return c[:k].reshape(n_bins, n_samples, 3), c[k:].reshape(n_bins, Engine.EDIT_POSITIONS, n_samples)
