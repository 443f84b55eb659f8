"""Host-side Python mirror of the reference's interface for the scoring hot path.

Thin layer over the C ABI (include/filtlong_hip.h) used by the tests and bench.py.  Names follow the
reference: ``Kmers`` (src/kmers.h:28-56), per-read scoring = the batched ``Read::Read``
(src/read.cpp:25-144), ``rank_and_cut`` = the global stage inlined in ``main`` (src/main.cpp:169-261).
All compute happens in the HIP library; there is no CPU fallback here.
"""
import ctypes as C
import traceback
import weakref

import numpy as np

from . import _lib
from ._lib import CutReport, FlxError, Params, Scores

CUT_NONE, CUT_NOT_ENOUGH, CUT_ALREADY_BELOW, CUT_SORTED = 0, 1, 2, 3


def make_params(window_size=250, min_length=None, max_length=None, min_mean_q=None, min_window_q=None, trim=False,
                split=None):
    """flx_params from keyword arguments named like the reference's CLI flags (src/arguments.cpp:152-205)."""
    p = Params()
    p.window_size = int(window_size)
    p.min_length_set, p.min_length = (1, int(min_length)) if min_length is not None else (0, 0)
    p.max_length_set, p.max_length = (1, int(max_length)) if max_length is not None else (0, 0)
    p.min_mean_q_set, p.min_mean_q = (1, float(min_mean_q)) if min_mean_q is not None else (0, 0.0)
    p.min_window_q_set, p.min_window_q = (1, float(min_window_q)) if min_window_q is not None else (0, 0.0)
    p.trim = 1 if trim else 0
    p.split_set, p.split = (1, int(split)) if split is not None else (0, 0)
    return p


def pack_reads(strings):
    """Pack byte strings into the 16-byte-aligned read plane of flx_score_batch.

    Returns (plane uint8[plane_bytes], offsets uint64[n], lengths int32[n])."""
    L = _lib.load()
    n = len(strings)
    lengths = np.array([len(s) for s in strings], dtype=np.int32)
    offsets = np.zeros(max(n, 1), dtype=np.uint64)
    pb = C.c_uint64()
    rc = L.flx_plane_layout(lengths.ctypes.data, n, offsets.ctypes.data, C.byref(pb))
    if rc:
        raise FlxError(rc, "flx_plane_layout")
    plane = np.zeros(pb.value, dtype=np.uint8)
    for s, o in zip(strings, offsets):
        if len(s):
            plane[int(o):int(o) + len(s)] = np.frombuffer(bytes(s), dtype=np.uint8)
    return plane, offsets[:n], lengths


def length_order(lengths):
    """Processing order: read indices by descending length (flx_length_order)."""
    L = _lib.load()
    lengths = np.ascontiguousarray(lengths, dtype=np.int32)
    order = np.zeros(max(len(lengths), 1), dtype=np.uint32)
    rc = L.flx_length_order(lengths.ctypes.data, len(lengths), order.ctypes.data)
    if rc:
        raise FlxError(rc, "flx_length_order")
    return order[:len(lengths)]


class Context:
    """One flx_ctx (one GPU).  Fails loudly without a gfx950 device."""

    def __init__(self, device=0):
        self.L = _lib.load()
        h = C.c_void_p()
        rc = self.L.flx_ctx_create(int(device), C.byref(h))
        if rc:
            raise FlxError(rc, self.L.flx_last_error(None).decode())
        self.h = h
        self._sets = []  # weak references to the Kmers created on this context (destroyed before the context)

    def close(self):
        if self.h:
            for ref in self._sets:
                ks = ref()
                if ks is not None:
                    ks.close()
            self._sets = []
            self.L.flx_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc:
            raise FlxError(rc, self.L.flx_last_error(self.h).decode())

    def device_info(self):
        name = C.create_string_buffer(256)
        ncu, mem = C.c_int(), C.c_uint64()
        self._check(self.L.flx_ctx_device_info(self.h, name, 256, C.byref(ncu), C.byref(mem)))
        return {"name": name.value.decode(), "n_cu": ncu.value, "hbm_bytes": mem.value}

    def set_stream(self, stream_ptr):
        self._check(self.L.flx_ctx_set_stream(self.h, C.c_void_p(stream_ptr)))

    def synchronize(self):
        self._check(self.L.flx_ctx_synchronize(self.h))

    # ---- timing ------------------------------------------------------------------------------
    def timing_enable(self, on=True):
        self._check(self.L.flx_timing_enable(self.h, 1 if on else 0))

    def timing_reset(self):
        self._check(self.L.flx_timing_reset(self.h))

    def timing_get(self, prefix=""):
        ms, n = C.c_double(), C.c_uint64()
        self._check(self.L.flx_timing_get(self.h, prefix.encode(), C.byref(ms), C.byref(n)))
        return ms.value, n.value

    # ---- seam 2: per-read scoring (host buffers) -----------------------------------------------
    def score_reads(self, plane, offsets, lengths, params, kmers=None, order=None, child_capacity=None, split_window_q=None,
                    adapters=None, seq_plane=None, trim_ends_q=None):
        """Batched Read::Read.  Returns a dict of numpy arrays in input order.  split_window_q (Phred mode only): the reads are
        split at their low-quality windows (flx_score_batch_qsplit).  adapters (an Adapters, Phred mode only) with seq_plane, the
        sequences at the offsets of the qualities: the adapters are cut off the read ends (flx_score_batch_adapters).  trim_ends_q
        (Phred mode only, a quality on the scale of min_window_q): the low-quality ends are cut off (flx_score_batch_endtrim with
        t = qsplit_threshold(trim_ends_q))."""
        if trim_ends_q is not None and (kmers is not None or split_window_q is not None or adapters is not None):
            raise ValueError("trim_ends_q is for Phred mode, and not with split_window_q or adapters")
        endtrim_t = None if trim_ends_q is None else qsplit_threshold(trim_ends_q)
        if split_window_q is not None and kmers is not None:
            raise ValueError("split_window_q is for Phred mode")
        if adapters is not None:
            if kmers is not None or split_window_q is not None:
                raise ValueError("adapters are for Phred mode, and not with split_window_q")
            seq_plane = np.ascontiguousarray(seq_plane, dtype=np.uint8)
            if seq_plane.nbytes != np.asarray(plane).nbytes:
                raise ValueError("the sequence plane must have the size of the quality plane")
        n = len(lengths)
        plane = np.ascontiguousarray(plane, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        lengths = np.ascontiguousarray(lengths, dtype=np.int32)
        out = {
            "mean_q": np.zeros(n, dtype=np.float64), "window_q": np.zeros(n, dtype=np.float64),
            "passed": np.zeros(n, dtype=np.uint8), "first": np.full(n, -1, dtype=np.int32),
            "last": np.full(n, -1, dtype=np.int32), "child_offsets": np.zeros(n + 1, dtype=np.uint64),
        }
        if child_capacity is None:
            child_capacity = max(16, 4 * n)
        ordp = None
        if order is not None:
            order = np.ascontiguousarray(order, dtype=np.uint32)
            ordp = order.ctypes.data
        while True:
            cr = np.zeros(2 * child_capacity, dtype=np.int32)
            cm = np.zeros(child_capacity, dtype=np.float64)
            cw = np.zeros(child_capacity, dtype=np.float64)
            cp = np.zeros(child_capacity, dtype=np.uint8)
            s = Scores()
            s.mean_q, s.window_q, s.passed = out["mean_q"].ctypes.data, out["window_q"].ctypes.data, out["passed"].ctypes.data
            s.first, s.last = out["first"].ctypes.data, out["last"].ctypes.data
            s.child_offsets = out["child_offsets"].ctypes.data
            s.child_ranges, s.child_mean_q, s.child_window_q, s.child_passed = (cr.ctypes.data, cm.ctypes.data,
                                                                              cw.ctypes.data, cp.ctypes.data)
            s.child_capacity = child_capacity
            if adapters is not None:
                rc = self.L.flx_score_batch_adapters(self.h, adapters.h, plane.ctypes.data, seq_plane.ctypes.data, plane.nbytes,
                                                     offsets.ctypes.data, lengths.ctypes.data, ordp, n, C.byref(params), C.byref(s))
            elif endtrim_t is not None:
                rc = self.L.flx_score_batch_endtrim(self.h, plane.ctypes.data, plane.nbytes, offsets.ctypes.data, lengths.ctypes.data,
                                                    ordp, n, C.byref(params), endtrim_t, C.byref(s))
            elif split_window_q is not None:
                rc = self.L.flx_score_batch_qsplit(self.h, plane.ctypes.data, plane.nbytes, offsets.ctypes.data, lengths.ctypes.data,
                                                   ordp, n, C.byref(params), float(split_window_q), C.byref(s))
            else:
                rc = self.L.flx_score_batch(self.h, kmers.h if kmers is not None else None, plane.ctypes.data,
                                            plane.nbytes, offsets.ctypes.data, lengths.ctypes.data, ordp, n,
                                            C.byref(params), C.byref(s))
            if rc == 5 and s.n_children > child_capacity:  # FLX_ERR_CAPACITY: retry with the reported size
                child_capacity = int(s.n_children)
                continue
            self._check(rc)
            break
        nc = int(s.n_children)
        out["child_ranges"] = cr[:2 * nc].reshape(-1, 2)
        out["child_mean_q"], out["child_window_q"], out["child_passed"] = cm[:nc], cw[:nc], cp[:nc]
        return out

    # ---- seam 2, streaming ----------------------------------------------------------------------
    def score_stream(self, chunks, params, kmers=None, chunk_bytes=1 << 20, chunk_reads=1 << 12, grow=False, split_window_q=None,
                     exclude=None, exclude_percent=10.0, adapters=None, max_low_complexity=None, low_complexity_score=20,
                     trim_ends_q=None):
        """flx_pipeline_*: `chunks` is an iterable of lists of byte strings (Phred mode: qualities, k-mer mode: sequences).
        Every chunk is packed into the pipeline's pinned buffer and submitted; returns the same dict as score_reads for
        all reads in submission order.  grow: enlarge the slots (flx_pipeline_reserve) for a chunk that does not fit.
        split_window_q: flx_pipeline_set_qsplit before the first chunk.  exclude (a Kmers filled with add_screen_fasta, or a
        ScreenSet): flx_pipeline_set_screen / flx_pipeline_set_screenset with exclude_percent; in Phred mode every chunk is then a PAIR (qualities, sequences) of lists, and
        the result also has "hits" and "excluded".  adapters (an Adapters, Phred mode): flx_pipeline_set_adapters; every chunk is
        such a PAIR as well and the result also has "adapter_keys" (n x 2: head, tail).  max_low_complexity (a percentage):
        flx_pipeline_set_complexity with low_complexity_score; in Phred mode every chunk is such a PAIR too, and the result also has
        "bad_windows" and "low_complexity".  trim_ends_q (Phred mode): flx_pipeline_set_endtrim before the first chunk; the result
        also has "endtrim_cuts" (n x 2: head, tail)."""
        L = self.L
        pipe = C.c_void_p()
        self._check(L.flx_pipeline_create(self.h, kmers.h if kmers is not None else None, C.byref(params), chunk_bytes,
                                          chunk_reads, C.byref(pipe)))
        try:
            if split_window_q is not None:
                self._check(L.flx_pipeline_set_qsplit(pipe, float(split_window_q)))
            two_planes = (exclude is not None or adapters is not None or max_low_complexity is not None) and (kmers is None or kmers.empty())
            if exclude is not None:
                set_screen = L.flx_pipeline_set_screenset if isinstance(exclude, ScreenSet) else L.flx_pipeline_set_screen
                self._check(set_screen(pipe, exclude.h, float(exclude_percent)))
            if adapters is not None:
                self._check(L.flx_pipeline_set_adapters(pipe, adapters.h))
            if max_low_complexity is not None:
                self._check(L.flx_pipeline_set_complexity(pipe, float(max_low_complexity), int(low_complexity_score)))
            if trim_ends_q is not None:
                self._check(L.flx_pipeline_set_endtrim(pipe, float(trim_ends_q)))
            for strings in chunks:
                seqs = None
                if two_planes:
                    strings, seqs = strings
                    assert [len(x) for x in strings] == [len(x) for x in seqs]
                n = len(strings)
                lengths = np.array([len(x) for x in strings], dtype=np.int32)
                offsets = np.zeros(max(n, 1), dtype=np.uint64)
                pb = C.c_uint64()
                self._check(L.flx_plane_layout(lengths.ctypes.data, n, offsets.ctypes.data, C.byref(pb)))
                if grow:
                    self._check(L.flx_pipeline_reserve(pipe, pb.value, n))
                buf, cap_b, cap_r = C.c_void_p(), C.c_uint64(), C.c_uint64()
                self._check(L.flx_pipeline_next_buffer(pipe, C.byref(buf), C.byref(cap_b), C.byref(cap_r)))
                if pb.value <= cap_b.value:  # an oversized chunk is submitted as is: the library must refuse it
                    view = np.ctypeslib.as_array(C.cast(buf, C.POINTER(C.c_uint8)), shape=(max(int(pb.value), 1),))
                    view[:pb.value] = 0
                    for x, o in zip(strings, offsets):
                        if len(x):
                            view[int(o):int(o) + len(x)] = np.frombuffer(bytes(x), dtype=np.uint8)
                    if seqs is not None and pb.value:  # the second plane: the sequences, at the same offsets
                        second = C.cast(C.c_void_p(buf.value + pb.value), C.POINTER(C.c_uint8))
                        view2 = np.ctypeslib.as_array(second, shape=(int(pb.value),))
                        view2[:] = 0
                        for x, o in zip(seqs, offsets):
                            if len(x):
                                view2[int(o):int(o) + len(x)] = np.frombuffer(bytes(x), dtype=np.uint8)
                self._check(L.flx_pipeline_submit(pipe, pb.value, offsets.ctypes.data, lengths.ctypes.data, n))
            s, n_all = Scores(), C.c_uint64()
            self._check(L.flx_pipeline_finish(pipe, C.byref(s), C.byref(n_all)))
            n, nc = int(n_all.value), int(s.n_children)

            def take(ptr, dtype, count):
                if count == 0:
                    return np.zeros(0, dtype=dtype)
                ct = np.ctypeslib.as_ctypes_type(dtype)
                return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(ct)), shape=(count,)).copy()

            out = {"mean_q": take(s.mean_q, np.float64, n), "window_q": take(s.window_q, np.float64, n),
                   "passed": take(s.passed, np.uint8, n), "first": take(s.first, np.int32, n),
                   "last": take(s.last, np.int32, n), "child_offsets": take(s.child_offsets, np.uint64, n + 1),
                   "child_ranges": take(s.child_ranges, np.int32, 2 * nc).reshape(-1, 2),
                   "child_mean_q": take(s.child_mean_q, np.float64, nc),
                   "child_window_q": take(s.child_window_q, np.float64, nc),
                   "child_passed": take(s.child_passed, np.uint8, nc)}
            if exclude is not None:
                hp, ep = C.c_void_p(), C.c_void_p()
                self._check(L.flx_pipeline_screen(pipe, C.byref(hp), C.byref(ep)))
                out["hits"], out["excluded"] = take(hp, np.uint32, n), take(ep, np.uint8, n)
            if max_low_complexity is not None:
                bp, fp = C.c_void_p(), C.c_void_p()
                self._check(L.flx_pipeline_complexity(pipe, C.byref(bp), C.byref(fp)))
                out["bad_windows"], out["low_complexity"] = take(bp, np.uint32, n), take(fp, np.uint8, n)
            if adapters is not None:
                kp = C.c_void_p()
                self._check(L.flx_pipeline_adapters(pipe, C.byref(kp)))
                out["adapter_keys"] = take(kp, np.uint32, 2 * n).reshape(-1, 2)
            if trim_ends_q is not None:
                cp = C.c_void_p()
                self._check(L.flx_pipeline_endtrim(pipe, C.byref(cp)))
                out["endtrim_cuts"] = take(cp, np.uint32, 2 * n).reshape(-1, 2)
            return out
        finally:
            L.flx_pipeline_destroy(pipe)

    # ---- seam 2, device-resident ---------------------------------------------------------------
    def score_reads_dev(self, d_plane, plane_bytes, d_offsets, d_lengths, d_order, n, params, d_mean_q, d_window_q,
                        d_passed, kmers=None):
        s = Scores()
        s.mean_q, s.window_q, s.passed = d_mean_q, d_window_q, d_passed
        self._check(self.L.flx_score_batch_dev(self.h, kmers.h if kmers is not None else None, d_plane, plane_bytes,
                                               d_offsets, d_lengths, d_order, n, C.byref(params), C.byref(s)))

    # ---- reads2 gather (src/main.cpp:138-147) ------------------------------------------------------
    def reads2_gather(self, lengths, scores):
        """flx_reads2_gather on the dictionary score_reads returns: file order, parents replaced in place by their children.
        Returns a dict of numpy arrays mean_q / window_q / length / passed / parent / child in reads2 order."""
        n = len(lengths)
        ln = np.ascontiguousarray(lengths, dtype=np.int32)
        nc = len(scores["child_mean_q"])
        keep = [np.ascontiguousarray(scores[k]) for k in ("mean_q", "window_q", "passed", "child_offsets", "child_ranges",
                                                          "child_mean_q", "child_window_q", "child_passed")]
        s = Scores()
        s.mean_q, s.window_q, s.passed, s.child_offsets = (keep[0].ctypes.data, keep[1].ctypes.data, keep[2].ctypes.data,
                                                           keep[3].ctypes.data)
        s.child_ranges, s.child_mean_q, s.child_window_q, s.child_passed = (keep[4].ctypes.data, keep[5].ctypes.data,
                                                                          keep[6].ctypes.data, keep[7].ctypes.data)
        s.child_capacity = s.n_children = nc
        cap = n + nc
        out = {"mean_q": np.zeros(cap, np.float64), "window_q": np.zeros(cap, np.float64), "length": np.zeros(cap, np.int32),
               "passed": np.zeros(cap, np.uint8), "parent": np.zeros(cap, np.uint32), "child": np.zeros(cap, np.int64)}
        n2 = C.c_uint64()
        self._check(self.L.flx_reads2_gather(self.h, n, ln.ctypes.data, C.byref(s), cap, out["mean_q"].ctypes.data,
                                             out["window_q"].ctypes.data, out["length"].ctypes.data, out["passed"].ctypes.data,
                                             out["parent"].ctypes.data, out["child"].ctypes.data, C.byref(n2)))
        return {k: v[:n2.value] for k, v in out.items()}

    def reads2_gather_dev(self, n, d_lengths, scores, capacity, d_mean2, d_window2, d_length2, d_passed2, d_parent2=None,
                          d_child2=None):
        """flx_reads2_gather_dev: `scores` is a _lib.Scores with device pointers (as filled by score_kmer_dev); returns n2."""
        n2 = C.c_uint64()
        self._check(self.L.flx_reads2_gather_dev(self.h, n, d_lengths, C.byref(scores), capacity, d_mean2, d_window2,
                                                 d_length2, d_passed2, d_parent2, d_child2, C.byref(n2)))
        return int(n2.value)

    # ---- seam 3: rank + cut --------------------------------------------------------------------
    def rank_and_cut(self, mean_q, window_q, length, passed, length_weight=1.0, mean_q_weight=1.0,
                     window_q_weight=1.0, target_bases=None, keep_percent=None, total_bases=None,
                     want_scores=True):
        n = len(mean_q)
        mq = np.ascontiguousarray(mean_q, dtype=np.float64)
        wq = np.ascontiguousarray(window_q, dtype=np.float64)
        ln = np.ascontiguousarray(length, dtype=np.int32)
        ps = np.array(passed, dtype=np.uint8)
        fs = np.zeros(n, dtype=np.float64) if want_scores else None
        if total_bases is None:
            total_bases = int(ln.astype(np.int64).sum())
        rep = CutReport()
        self._check(self.L.flx_rank_and_cut(self.h, n, mq.ctypes.data, wq.ctypes.data, ln.ctypes.data, ps.ctypes.data,
                                            length_weight, mean_q_weight, window_q_weight,
                                            1 if target_bases is not None else 0, int(target_bases or 0),
                                            1 if keep_percent is not None else 0, float(keep_percent or 0.0),
                                            int(total_bases), fs.ctypes.data if want_scores else None, C.byref(rep)))
        return {"passed": ps, "final_score": fs, "report": rep}

    def rank_and_cut_dev(self, n, d_mean_q, d_window_q, d_length, d_passed, length_weight=1.0, mean_q_weight=1.0,
                         window_q_weight=1.0, target_bases=None, keep_percent=None, total_bases=0,
                         d_final_score=None):
        rep = CutReport()
        self._check(self.L.flx_rank_and_cut_dev(self.h, n, d_mean_q, d_window_q, d_length, d_passed, length_weight,
                                                mean_q_weight, window_q_weight,
                                                1 if target_bases is not None else 0, int(target_bases or 0),
                                                1 if keep_percent is not None else 0, float(keep_percent or 0.0),
                                                int(total_bases), d_final_score, C.byref(rep)))
        return rep

    def rank_and_cut_sharded_dev(self, n_total, d_mean_q_all, first, n_local, d_window_q, d_length, d_passed, rank, world,
                                 reduce=None, length_weight=1.0, mean_q_weight=1.0, window_q_weight=1.0,
                                 target_bases=None, keep_percent=None, total_bases=0, d_final_score=None):
        """flx_rank_and_cut_sharded_dev.  `reduce(buf)` receives a writable numpy uint64 view of the library's host
        buffer and must replace it by its sum over all ranks (filtlong_amd.dist.make_reduce builds one over
        torch.distributed).  Returns (report, need_replicated)."""
        rep = CutReport()

        def _cb(_user, buf, count):
            try:
                reduce(np.ctypeslib.as_array(buf, shape=(int(count),)))
                return 0
            except Exception:  # an exception must not unwind through the C frames
                traceback.print_exc()
                return 1
        cb = _lib.ALLREDUCE_FN(_cb) if reduce is not None else C.cast(None, _lib.ALLREDUCE_FN)
        rc = self.L.flx_rank_and_cut_sharded_dev(self.h, n_total, d_mean_q_all, first, n_local, d_window_q, d_length, d_passed,
                                                 length_weight, mean_q_weight, window_q_weight,
                                                 1 if target_bases is not None else 0, int(target_bases or 0),
                                                 1 if keep_percent is not None else 0, float(keep_percent or 0.0),
                                                 int(total_bases), d_final_score, rank, world, cb, None, C.byref(rep))
        if rc == _lib.NEED_REPLICATED:
            return rep, True
        self._check(rc)
        return rep, False

    # ---- multi-GPU with the library's own RCCL communicator (include/filtlong_hip.h, flx_comm_*) -------------------
    def comm_unique_id(self):
        buf = C.create_string_buffer(128)
        self._check(self.L.flx_comm_unique_id(self.h, buf))
        return buf.raw

    def comm_init(self, unique_id, rank, world):
        self._check(self.L.flx_comm_init(self.h, C.c_char_p(bytes(unique_id)), rank, world))

    def comm_destroy(self):
        self._check(self.L.flx_comm_destroy(self.h))

    def comm_sum_u64(self, values):
        a = np.ascontiguousarray(values, dtype=np.uint64).copy()
        self._check(self.L.flx_comm_sum_u64(self.h, a.ctypes.data, a.size))
        return a

    def rank_and_cut_comm(self, mean_q, window_q, length, passed, length_weight=1.0, mean_q_weight=1.0, window_q_weight=1.0,
                          target_bases=None, keep_percent=None, total_bases=0, want_scores=False):
        """flx_rank_and_cut_comm: this rank's reads2 scalars as host arrays (what the CLI holds); `total_bases` is the global
        sum.  Returns the same dictionary as rank_and_cut for the local block."""
        n = len(mean_q)
        mq = np.ascontiguousarray(mean_q, dtype=np.float64)
        wq = np.ascontiguousarray(window_q, dtype=np.float64)
        ln = np.ascontiguousarray(length, dtype=np.int32)
        ps = np.array(passed, dtype=np.uint8)
        fs = np.zeros(n, dtype=np.float64) if want_scores else None
        rep = CutReport()
        self._check(self.L.flx_rank_and_cut_comm(self.h, n, mq.ctypes.data, wq.ctypes.data, ln.ctypes.data, ps.ctypes.data,
                                                 length_weight, mean_q_weight, window_q_weight,
                                                 1 if target_bases is not None else 0, int(target_bases or 0),
                                                 1 if keep_percent is not None else 0, float(keep_percent or 0.0),
                                                 int(total_bases), fs.ctypes.data if want_scores else None, C.byref(rep)))
        return {"passed": ps, "final_score": fs, "report": rep}

    def rank_and_cut_comm_dev(self, n_local, d_mean_q, d_window_q, d_length, d_passed, length_weight=1.0, mean_q_weight=1.0,
                              window_q_weight=1.0, target_bases=None, keep_percent=None, total_bases=0, d_final_score=None):
        """flx_rank_and_cut_comm_dev: the global stage over all ranks of the context's RCCL communicator (one all-gather of
        the mean qualities + device-side all-reduces, no host round trips per pass); `total_bases` is the global sum."""
        rep = CutReport()
        self._check(self.L.flx_rank_and_cut_comm_dev(self.h, n_local, d_mean_q, d_window_q, d_length, d_passed, length_weight,
                                                     mean_q_weight, window_q_weight, 1 if target_bases is not None else 0,
                                                     int(target_bases or 0), 1 if keep_percent is not None else 0,
                                                     float(keep_percent or 0.0), int(total_bases), d_final_score, C.byref(rep)))
        return rep

    # ---- the contaminant screen ------------------------------------------------------------------
    def _per_read(self, fn, handle, plane, offsets, lengths, order, per_read):
        """The host-array form of a call that answers `per_read` uint32 per read of the SEQUENCE plane, in input order."""
        n = len(lengths)
        plane = np.ascontiguousarray(plane, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        lengths = np.ascontiguousarray(lengths, dtype=np.int32)
        out = np.full(per_read * max(n, 1), 0xA5A5A5A5, dtype=np.uint32)
        ordp = None
        if order is not None:
            order = np.ascontiguousarray(order, dtype=np.uint32)
            ordp = order.ctypes.data
        self._check(fn(self.h, handle, plane.ctypes.data, plane.nbytes, offsets.ctypes.data, lengths.ctypes.data, ordp, n, out.ctypes.data))
        return out[:per_read * n]

    def screen_hits(self, plane, offsets, lengths, kmers, order=None):
        """flx_screen_hits: for every read of the SEQUENCE plane the number of its 16-mers that are members of `kmers` (a set
        filled with Kmers.add_screen_fasta).  uint32 array in input order."""
        return self._per_read(self.L.flx_screen_hits, kmers.h, plane, offsets, lengths, order, 1)

    def screenset_hits(self, plane, offsets, lengths, sset, order=None):
        """flx_screenset_hits: screen_hits against a ScreenSet — the number of every read's K-mers (K = sset.k) whose canonical key
        is stored in it.  uint32 array in input order."""
        return self._per_read(self.L.flx_screenset_hits, sset.h, plane, offsets, lengths, order, 1)

    def screen_hits_dev(self, kmers, d_plane, plane_bytes, d_offsets, d_lengths, d_order, n, d_hits):
        self._check(self.L.flx_screen_hits_dev(self.h, kmers.h, d_plane, plane_bytes, d_offsets, d_lengths, d_order, n, d_hits))

    # ---- the low-complexity filter ---------------------------------------------------------------
    def complexity_bad(self, plane, offsets, lengths, score=20, order=None):
        """flx_complexity_bad: for every read of the SEQUENCE plane the number of its 64-base windows whose triplet-pair score S has
        10 S > score * 61 (windows with a byte outside ACGTacgt are never bad).  uint32 array in input order."""
        n = len(lengths)
        plane = np.ascontiguousarray(plane, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        lengths = np.ascontiguousarray(lengths, dtype=np.int32)
        out = np.full(max(n, 1), 0xA5A5A5A5, dtype=np.uint32)
        ordp = None
        if order is not None:
            order = np.ascontiguousarray(order, dtype=np.uint32)
            ordp = order.ctypes.data
        self._check(self.L.flx_complexity_bad(self.h, plane.ctypes.data, plane.nbytes, offsets.ctypes.data, lengths.ctypes.data, ordp, n,
                                              int(score), out.ctypes.data))
        return out[:n]

    def complexity_bad_dev(self, d_plane, plane_bytes, d_offsets, d_lengths, d_order, n, score, d_bad):
        self._check(self.L.flx_complexity_bad_dev(self.h, d_plane, plane_bytes, d_offsets, d_lengths, d_order, n, int(score), d_bad))

    # ---- quality trimming of the read ends -----------------------------------------------------------
    def endtrim_cuts(self, plane, offsets, lengths, t, order=None):
        """flx_endtrim_cuts: for every read of the QUALITY plane its head cut and its tail cut against the threshold t (0 <= t < 2^32
        on the scale of qsplit_table(); qsplit_threshold(Q) for a quality Q).  uint32 array (n, 2) in input order."""
        n = len(lengths)
        plane = np.ascontiguousarray(plane, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        lengths = np.ascontiguousarray(lengths, dtype=np.int32)
        out = np.full(2 * max(n, 1), 0xA5A5A5A5, dtype=np.uint32)
        ordp = None
        if order is not None:
            order = np.ascontiguousarray(order, dtype=np.uint32)
            ordp = order.ctypes.data
        self._check(self.L.flx_endtrim_cuts(self.h, plane.ctypes.data, plane.nbytes, offsets.ctypes.data, lengths.ctypes.data, ordp, n,
                                            int(t), out.ctypes.data))
        return out[:2 * n].reshape(-1, 2)

    def endtrim_cuts_dev(self, d_plane, plane_bytes, d_offsets, d_lengths, d_order, n, t, d_cuts):
        self._check(self.L.flx_endtrim_cuts_dev(self.h, d_plane, plane_bytes, d_offsets, d_lengths, d_order, n, int(t), d_cuts))

    # ---- adapter trimming -------------------------------------------------------------------------
    def adapter_cuts(self, plane, offsets, lengths, adapters, order=None):
        """flx_adapter_cuts: for every read of the SEQUENCE plane its two keys, (jbest << 8) | pattern of the adapter occurrence that
        reaches furthest into the read at the head and at the tail, 0 without a hit.  uint32 array (n, 2) in input order."""
        return self._per_read(self.L.flx_adapter_cuts, adapters.h, plane, offsets, lengths, order, 2).reshape(-1, 2)

    def adapter_cuts_dev(self, adapters, d_plane, plane_bytes, d_offsets, d_lengths, d_order, n, d_keys):
        self._check(self.L.flx_adapter_cuts_dev(self.h, adapters.h, d_plane, plane_bytes, d_offsets, d_lengths, d_order, n, d_keys))

    def adapter_marks(self, plane, offsets, lengths, adapters, order=None, bitmap=False):
        """flx_adapter_marks (adapters with split_errors set): the bases of every read that lie in an adapter occurrence inside it.
        A list of boolean arrays, one per read in input order; bitmap=True: the uint32 words over the plane as the library returns
        them, bit offsets[i] + b for base b of read i."""
        n = len(lengths)
        plane = np.ascontiguousarray(plane, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        lengths = np.ascontiguousarray(lengths, dtype=np.int32)
        words = np.full(max((plane.nbytes + 31) // 32, 1), 0xA5A5A5A5, dtype=np.uint32)
        ordp = None
        if order is not None:
            order = np.ascontiguousarray(order, dtype=np.uint32)
            ordp = order.ctypes.data
        self._check(self.L.flx_adapter_marks(self.h, adapters.h, plane.ctypes.data, plane.nbytes, offsets.ctypes.data, lengths.ctypes.data,
                                             ordp, n, words.ctypes.data))
        if bitmap:
            return words
        bits = np.unpackbits(words.view(np.uint8), bitorder="little")
        return [bits[int(o):int(o) + int(l)].astype(bool) for o, l in zip(offsets, lengths)]

    def adapter_marks_dev(self, adapters, d_plane, plane_bytes, d_offsets, d_lengths, d_order, n, d_marks):
        self._check(self.L.flx_adapter_marks_dev(self.h, adapters.h, d_plane, plane_bytes, d_offsets, d_lengths, d_order, n, d_marks))

    def last_screen_filter(self):
        """"lds", "pre12" or "exact": the filter in front of the exact bitmap in the last screen_hits call."""
        return self.L.flx_last_screen_filter(self.h).decode()

    def last_phred_kernel(self):
        return self.L.flx_last_phred_kernel(self.h).decode()

    def last_kmer_cover(self):
        """"q", "w" or "v2": the coverage kernel the last k-mer scoring call launched."""
        return self.L.flx_last_kmer_cover(self.h).decode()

    def last_kmer_handed_over(self):
        """Reads of the last k-mer scoring call that went to the kernel with a diagonal per lane (insertions / deletions)."""
        return int(self.L.flx_last_kmer_handed_over(self.h))

    def last_kmer_locus(self):
        return bool(self.L.flx_last_kmer_locus(self.h))

    def last_kmer_fold_grid(self):
        return bool(self.L.flx_last_kmer_fold_grid(self.h))

    def synth_qual_dev(self, seed, d_plane, plane_bytes, d_offsets, d_lengths, d_read_ids, n, profile=0):
        self._check(self.L.flx_synth_qual_profile_dev(self.h, seed, profile, d_plane, plane_bytes, d_offsets, d_lengths,
                                                      d_read_ids, n))

    def synth_seq_dev(self, seed, d_plane, plane_bytes, d_offsets, d_lengths, d_read_ids, n, d_ref, ref_len, profile=0):
        self._check(self.L.flx_synth_seq_profile_dev(self.h, seed, int(profile), d_plane, plane_bytes, d_offsets, d_lengths, d_read_ids, n, d_ref,
                                                     ref_len))

    def score_kmer_dev(self, kmers, d_plane, plane_bytes, d_offsets, d_lengths, d_order, n, params, scores):
        """flx_score_batch_dev in k-mer mode; `scores` is a filled _lib.Scores with device pointers."""
        rc = self.L.flx_score_batch_dev(self.h, kmers.h, d_plane, plane_bytes, d_offsets, d_lengths, d_order, n,
                                        C.byref(params), C.byref(scores))
        if rc != 5:
            self._check(rc)
        return rc


    def bgzf_compress_dev(self, d_in, n, d_out, out_cap, eof=True):
        """flx_bgzf_compress_dev: BGZF of the n device bytes at d_in into d_out (device, out_cap bytes) -> bytes written."""
        got = C.c_uint64()
        self._check(self.L.flx_bgzf_compress_dev(self.h, d_in, int(n), BGZF_EOF if eof else 0, d_out, int(out_cap), C.byref(got)))
        return got.value

    def bgzf_inflate_dev(self, d_in, d_in_off, d_out_off, n_members, d_out, d_status):
        """flx_bgzf_inflate_dev: member k = bytes [d_in_off[k], d_in_off[k+1]) of d_in to [d_out_off[k], d_out_off[k+1]) of d_out
        (device pointers; offsets uint64, n_members + 1 each; d_status uint32) -> the lowest member that is not ok, or n_members."""
        first_bad = C.c_uint64()
        self._check(self.L.flx_bgzf_inflate_dev(self.h, d_in, d_in_off, d_out_off, int(n_members), d_out, d_status, C.byref(first_bad)))
        return first_bad.value

    def bam_to_fastq_dev(self, d_bam, n, d_rec_off, n_records, d_out, out_cap, d_out_off):
        """flx_bam_to_fastq_dev: records [d_rec_off[k], d_rec_off[k+1]) of the n device bytes at d_bam as FASTQ text into d_out
        (device, out_cap bytes); d_out_off (device, uint64, n_records + 1) gets the text offsets -> (out_len, n_skipped, first_bad).
        FLX_ERR_CAPACITY raises FlxError with the length needed in its `needed`."""
        out_len, skipped, first_bad = C.c_uint64(), C.c_uint64(), C.c_uint64()
        rc = self.L.flx_bam_to_fastq_dev(self.h, d_bam, int(n), d_rec_off, int(n_records), d_out, int(out_cap), d_out_off,
                                         C.byref(out_len), C.byref(skipped), C.byref(first_bad))
        if rc:
            e = FlxError(rc, self.L.flx_last_error(self.h).decode())
            e.needed = out_len.value
            raise e
        return out_len.value, skipped.value, first_bad.value

    def bam_from_fastq_dev(self, d_text, n, d_rec_off, n_records, d_out, out_cap, d_out_off):
        """flx_bam_from_fastq_dev: the strict FASTQ / FASTA records [d_rec_off[k], d_rec_off[k+1]) of the n device bytes at d_text as
        unaligned BAM records into d_out (device, out_cap bytes); d_out_off (device, uint64, n_records + 1) gets their offsets ->
        (out_len, first_bad).  FLX_ERR_CAPACITY raises FlxError with the length needed in its `needed`."""
        out_len, first_bad = C.c_uint64(), C.c_uint64()
        rc = self.L.flx_bam_from_fastq_dev(self.h, d_text, int(n), d_rec_off, int(n_records), d_out, int(out_cap), d_out_off,
                                           C.byref(out_len), C.byref(first_bad))
        if rc:
            e = FlxError(rc, self.L.flx_last_error(self.h).decode())
            e.needed = out_len.value
            raise e
        return out_len.value, first_bad.value

    # ---- read summary (include/filtlong_hip.h, flx_summary*) ------------------------------------------------------
    def summary(self, lengths, mean_q=None, window_q=None, mask=None, global_=False):
        """flx_summary over host arrays: the struct's fields as a dictionary (integers and lists of integers).  `mask`:
        entries with a non-zero byte count (None: all).  global_: collective over the context's communicator."""
        ln = np.ascontiguousarray(lengths, dtype=np.int32)
        n = len(ln)
        mq = None if mean_q is None else np.ascontiguousarray(mean_q, dtype=np.float64)
        wq = None if window_q is None else np.ascontiguousarray(window_q, dtype=np.float64)
        mk = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
        for a in (mq, wq, mk):
            if a is not None and len(a) != n:
                raise ValueError("summary: arrays of different lengths")
        out = _lib.Summary()
        self._check(self.L.flx_summary(self.h, n, ln.ctypes.data, None if mq is None else mq.ctypes.data,
                                       None if wq is None else wq.ctypes.data, None if mk is None else mk.ctypes.data,
                                       1 if global_ else 0, C.byref(out)))
        return summary_dict(out)

    def summary_dev(self, n, d_length, d_mean_q=None, d_window_q=None, d_mask=None, global_=False):
        """flx_summary_dev: the same over device pointers (int32 lengths, float64 qualities, uint8 mask)."""
        out = _lib.Summary()
        self._check(self.L.flx_summary_dev(self.h, int(n), d_length, d_mean_q, d_window_q, d_mask, 1 if global_ else 0,
                                           C.byref(out)))
        return summary_dict(out)


SUMMARY_FIELDS = ("n", "bases", "min_length", "max_length", "median_length", "nx", "len_count", "len_bases",
                  "mean_q_count", "mean_q_bases", "window_q_count", "window_q_bases")


def qsplit_table():
    """E[0..255] of --split_window_q (flx_qsplit_table; no device needed)."""
    e = np.zeros(256, dtype=np.uint32)
    rc = _lib.load().flx_qsplit_table(e.ctypes.data)
    if rc:
        raise FlxError(rc, "flx_qsplit_table")
    return e


def qsplit_threshold(q):
    """t of --split_window_q q (flx_qsplit_threshold; no device needed)."""
    t = C.c_uint64()
    rc = _lib.load().flx_qsplit_threshold(float(q), C.byref(t))
    if rc:
        raise FlxError(rc, "split_window_q must be greater than 0 and less than 100")
    return int(t.value)


def endtrim_span():
    """Quality bytes per work item of the end-trimming kernel (flx_endtrim_span; no device needed)."""
    return int(_lib.load().flx_endtrim_span())


def screen_threshold(percent):
    """t of --exclude_percent P (flx_screen_threshold; no device needed)."""
    t = C.c_uint64()
    rc = _lib.load().flx_screen_threshold(float(percent), C.byref(t))
    if rc:
        raise FlxError(rc, "exclude_percent must be greater than 0 and at most 100")
    return int(t.value)


def screen_span():
    """Window positions per work item of the screen kernel (flx_screen_span; no device needed)."""
    return int(_lib.load().flx_screen_span())


def screen_excluded(hits, lengths, percent):
    """The decision of --exclude on integers: windows > 0 and (hits << 32) >= t * windows."""
    t = screen_threshold(percent)
    out = np.zeros(len(hits), dtype=np.uint8)
    for i, (h, n) in enumerate(zip(hits, lengths)):
        w = max(0, int(n) - 15)
        out[i] = 1 if w > 0 and (int(h) << 32) >= t * w else 0
    return out


def complexity_window():
    """Bases of a window of the low-complexity filter: 64 (flx_complexity_window; no device needed)."""
    return int(_lib.load().flx_complexity_window())


def complexity_span():
    """Window positions per work item of the low-complexity kernel (flx_complexity_span; no device needed)."""
    return int(_lib.load().flx_complexity_span())


def complexity_flagged(bad, lengths, percent):
    """The decision of --max_low_complexity on integers: windows > 0 and (bad << 32) >= t * windows, windows = max(0, L - 63)."""
    t = screen_threshold(percent)
    out = np.zeros(len(bad), dtype=np.uint8)
    for i, (b, n) in enumerate(zip(bad, lengths)):
        w = max(0, int(n) - 63)
        out[i] = 1 if w > 0 and (int(b) << 32) >= t * w else 0
    return out


def summary_dict(s):
    """struct flx_summary -> {field: int or list of ints} (padding left out)."""
    d = {}
    for name in SUMMARY_FIELDS:
        v = getattr(s, name)
        d[name] = int(v) if isinstance(v, int) else [int(x) for x in v]
    return d


def summary_q_edges():
    """The 51 quality-bin edges of flx_summary, edges[k] = 100 (1 - 10^(-k/10)): the very doubles the kernel bins with."""
    e = np.zeros(51, dtype=np.float64)
    rc = _lib.load().flx_summary_q_edges(e.ctypes.data)
    if rc:
        raise FlxError(rc, "flx_summary_q_edges")
    return e


BGZF_EOF = 1  # FLX_BGZF_EOF


def bgzf_bound(n, eof=True):
    """The most bytes a BGZF compression of n bytes writes (flx_bgzf_bound)."""
    b = C.c_uint64()
    rc = _lib.load().flx_bgzf_bound(int(n), BGZF_EOF if eof else 0, C.byref(b))
    if rc:
        raise FlxError(rc, "flx_bgzf_bound")
    return b.value


def bgzf_index(data, max_members=None):
    """flx_bgzf_index (host only): the well-formed BGZF members at the front of `data` -> (in_off, out_off), two uint64 arrays of
    members + 1 prefix sums: member k is data[in_off[k]:in_off[k+1]] and holds out_off[k+1] - out_off[k] bytes."""
    src = np.frombuffer(bytes(data), dtype=np.uint8)
    cap = len(src) // 26 + 1 if max_members is None else int(max_members)
    in_off = np.zeros(cap + 1, dtype=np.uint64)
    out_off = np.zeros(cap + 1, dtype=np.uint64)
    m = C.c_uint64()
    rc = _lib.load().flx_bgzf_index(src.ctypes.data if len(src) else None, len(src), cap, in_off.ctypes.data, out_off.ctypes.data,
                                    C.byref(m))
    if rc:
        raise FlxError(rc, "flx_bgzf_index")
    return in_off[:m.value + 1].copy(), out_off[:m.value + 1].copy()


BAM_END, BAM_TRUNCATED, BAM_MALFORMED, BAM_HEADER, BAM_MORE = range(5)  # FLX_BAM_*: why flx_bam_index stopped


def bam_index(data, max_records=None):
    """flx_bam_index (host only) over inflated BAM bytes -> (rec_off, end_state): record k is data[rec_off[k]:rec_off[k+1]]
    (rec_off[0] is the end of the header) and end_state one of the BAM_* values above."""
    src = np.frombuffer(bytes(data), dtype=np.uint8)
    cap = len(src) // 36 + 1 if max_records is None else int(max_records)
    rec_off = np.zeros(cap + 1, dtype=np.uint64)
    m, end = C.c_uint64(), C.c_int()
    rc = _lib.load().flx_bam_index(src.ctypes.data if len(src) else None, len(src), cap, rec_off.ctypes.data, C.byref(m), C.byref(end))
    if rc:
        raise FlxError(rc, "flx_bam_index")
    return rec_off[:m.value + 1].copy(), end.value


def bam_to_fastq(ctx, data, piece_bytes=0, out_cap=None, with_offsets=False):
    """flx_bam_to_fastq: inflated BAM bytes in, FASTQ bytes out (the records bam_index finds; a truncated or malformed file raises
    ValueError).  with_offsets: -> (bytes, text offsets of the records, skipped records)."""
    src = np.frombuffer(bytes(data), dtype=np.uint8)
    rec_off, end = bam_index(src)
    if end != BAM_END:
        raise ValueError("bam_to_fastq: %s at record %d" % ({BAM_TRUNCATED: "truncated", BAM_MALFORMED: "malformed", BAM_HEADER: "bad header"}.get(end, end),
                                                            len(rec_off) - 1))
    n = len(rec_off) - 1
    cap = 2 * int(rec_off[n] - rec_off[0]) if out_cap is None else int(out_cap)
    out = np.empty(max(cap, 1), dtype=np.uint8)
    out_off = np.zeros(n + 1, dtype=np.uint64)
    out_len, skipped, first_bad = C.c_uint64(), C.c_uint64(), C.c_uint64()
    rc = ctx.L.flx_bam_to_fastq(ctx.h, src.ctypes.data if len(src) else None, len(src), rec_off.ctypes.data, n, int(piece_bytes),
                                out.ctypes.data, cap, out_off.ctypes.data, C.byref(out_len), C.byref(skipped), C.byref(first_bad))
    if rc:
        e = FlxError(rc, ctx.L.flx_last_error(ctx.h).decode())
        e.needed = out_len.value
        raise e
    if first_bad.value != n:
        raise ValueError("bam_to_fastq: record %d is malformed" % first_bad.value)
    text = out[:out_len.value].tobytes()
    return (text, out_off, skipped.value) if with_offsets else text


def bam_header():
    """flx_bam_header: the header bytes of a BAM file written from text."""
    n = C.c_uint64()
    L = _lib.load()
    L.flx_bam_header(None, 0, C.byref(n))
    out = np.zeros(n.value, dtype=np.uint8)
    rc = L.flx_bam_header(out.ctypes.data, len(out), C.byref(n))
    if rc:
        raise FlxError(rc, "flx_bam_header")
    return out.tobytes()


def bam_from_fastq_bound(n_text, n_records):
    """flx_bam_from_fastq_bound: the most BAM bytes n_records records in n_text bytes of text can take."""
    b = C.c_uint64()
    rc = _lib.load().flx_bam_from_fastq_bound(int(n_text), int(n_records), C.byref(b))
    if rc:
        raise FlxError(rc, "flx_bam_from_fastq_bound")
    return b.value


def _text_and_offsets(text, rec_off):
    src = np.frombuffer(bytes(text), dtype=np.uint8)
    off = np.ascontiguousarray(rec_off, dtype=np.uint64)
    if len(off) < 1:
        raise ValueError("rec_off needs n_records + 1 entries")
    return src, off


def bam_from_fastq(ctx, text, rec_off, with_offsets=False):
    """Strict FASTQ / FASTA record text (record k is text[rec_off[k]:rec_off[k+1]]) -> the BAM records, without a header, through
    flx_bam_from_fastq_dev (device buffers from torch).  An invalid record raises ValueError.  with_offsets: -> (bytes, offsets)."""
    import torch
    src, off = _text_and_offsets(text, rec_off)
    n = len(off) - 1
    if n == 0:
        return (b"", [0]) if with_offsets else b""
    cap = bam_from_fastq_bound(len(src), n)
    d_text = torch.from_numpy(src.copy()).to("cuda") if len(src) else torch.zeros(1, dtype=torch.uint8, device="cuda")
    d_off = torch.from_numpy(off.view(np.int64).copy()).to("cuda")
    d_out = torch.empty(cap + 16, dtype=torch.uint8, device="cuda")
    d_oo = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    out_len, first_bad = ctx.bam_from_fastq_dev(d_text.data_ptr(), len(src), d_off.data_ptr(), n, d_out.data_ptr(), cap, d_oo.data_ptr())
    if first_bad != n:
        raise ValueError("bam_from_fastq: record %d is not valid" % first_bad)
    data = d_out[:out_len].cpu().numpy().tobytes()
    return (data, [int(x) for x in d_oo.cpu().numpy()]) if with_offsets else data


def bgzf_bam_from_fastq(bgzf, text, rec_off, eof=True, out_cap=None):
    """flx_bgzf_bam_from_fastq through a slot of the Bgzf object: strict record text in, BGZF-compressed BAM records (no header)
    out -> bytes.  An invalid record raises ValueError."""
    src, off = _text_and_offsets(text, rec_off)
    n = len(off) - 1
    cap = bgzf_bound(bam_from_fastq_bound(len(src), n), eof) + 31 * n if out_cap is None else int(out_cap)
    out = np.empty(max(cap, 1), dtype=np.uint8)
    got, first_bad = C.c_uint64(), C.c_uint64()
    rc = bgzf.ctx.L.flx_bgzf_bam_from_fastq(bgzf.h, src.ctypes.data if len(src) else None, len(src), off.ctypes.data, n,
                                            BGZF_EOF if eof else 0, out.ctypes.data, cap, C.byref(got), C.byref(first_bad))
    if rc:
        raise FlxError(rc, "flx_bgzf_bam_from_fastq")
    if first_bad.value != n:
        raise ValueError("bgzf_bam_from_fastq: record %d is not valid" % first_bad.value)
    return out[:got.value].tobytes()


class Bgzf:
    """Host-to-host BGZF compressor (flx_bgzf) with `slots` pinned slots of `slot_bytes`; compress() may be called from
    several threads at once (ctypes releases the GIL for the call)."""

    def __init__(self, ctx, slot_bytes=16 << 20, slots=4):
        self.ctx = ctx
        h = C.c_void_p()
        ctx._check(ctx.L.flx_bgzf_create(ctx.h, int(slot_bytes), int(slots), C.byref(h)))
        self.h = h
        ctx._sets.append(weakref.ref(self))

    def compress(self, data, eof=True, out_cap=None):
        src = np.frombuffer(bytes(data), dtype=np.uint8)
        cap = bgzf_bound(len(src), eof) if out_cap is None else int(out_cap)
        out = np.empty(max(cap, 1), dtype=np.uint8)
        got = C.c_uint64()
        rc = self.ctx.L.flx_bgzf_compress(self.h, src.ctypes.data if len(src) else None, len(src), BGZF_EOF if eof else 0,
                                          out.ctypes.data, cap, C.byref(got))
        if rc:
            raise FlxError(rc, "flx_bgzf_compress")
        return out[:got.value].tobytes()

    def inflate(self, data):
        """flx_bgzf_inflate of the BGZF members at the front of `data` (those bgzf_index finds) -> (bytes, first_bad): the bytes
        of the members in front of the first bad one, and its index (the number of members when all are ok)."""
        src = np.frombuffer(bytes(data), dtype=np.uint8)
        in_off, out_off = bgzf_index(src)
        n = len(in_off) - 1
        out = np.empty(max(int(out_off[n]), 1), dtype=np.uint8)
        first_bad = C.c_uint64()
        rc = self.ctx.L.flx_bgzf_inflate(self.h, src.ctypes.data if len(src) else None, in_off.ctypes.data, out_off.ctypes.data, n,
                                         out.ctypes.data, C.byref(first_bad))
        if rc:
            raise FlxError(rc, "flx_bgzf_inflate")
        return out[:int(out_off[first_bad.value])].tobytes(), first_bad.value

    def close(self):
        if self.h:
            if self.ctx.h:  # destroyed before its context (Context.close() closes it first)
                self.ctx.L.flx_bgzf_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Adapters:
    """flx_adapters: the sequences of --trim_adapters (12 to 64 bases of ACGT each, at most 128), each with its reverse complement;
    errors: the edits a pattern may carry, percent of its length (0..40); window: the bases at either read end that are searched
    (1..1024).  split_errors (0..40, None: off): the adapters INSIDE the reads are searched as well, with that many edits percent, and
    the reads are split there (flx_adapters_set_split).  overhang (0..52, 0: off): an adapter that the read begins or ends inside is
    found as well, with up to that many of its bases missing beyond the read's edge (flx_adapters_set_overhang).  Belongs to no
    context."""

    def __init__(self, seqs, errors=20, window=150, split_errors=None, overhang=0):
        seqs = [bytes(s) for s in seqs]
        n = len(seqs)
        lengths = np.array([len(s) for s in seqs], dtype=np.int64)
        offsets = np.zeros(max(n, 1), dtype=np.uint64)
        if n:
            offsets[1:n] = np.cumsum(lengths[:-1])
        bases = np.frombuffer(b"".join(seqs) or b"\0", dtype=np.uint8)
        self.L = _lib.load()
        h = C.c_void_p()
        rc = self.L.flx_adapters_create(bases.ctypes.data, offsets.ctypes.data, lengths.ctypes.data, n, int(errors), int(window), C.byref(h))
        if rc != _lib.FLX_OK:
            raise FlxError(rc, "flx_adapters_create: 1 to 128 sequences of 12 to 64 bases of ACGT, errors 0..40, window 1..1024")
        self.h = h
        self.errors, self.window = int(errors), int(window)
        self.split_errors = None
        if split_errors is not None:
            self.set_split(split_errors)
        self._overhang = 0
        if overhang != 0:  # (0 is the state after flx_adapters_create)
            self.overhang = overhang

    @property
    def overhang(self):
        """flx_adapters_overhang: the adapter bases that may lie beyond a read's edge, 0: the whole adapter must be in the read"""
        return self._overhang

    @overhang.setter
    def overhang(self, overhang):
        """flx_adapters_set_overhang: 0..52; the devices that hold the patterns get them again with their next call"""
        if self.L.flx_adapters_set_overhang(self.h, int(overhang)) != _lib.FLX_OK:
            raise FlxError(1, "flx_adapters_set_overhang: overhang 0..52")
        self._overhang = int(self.L.flx_adapters_overhang(self.h))

    def set_split(self, split_errors):
        """flx_adapters_set_split: 0..40 turns the search inside the reads on, None (or -1) off"""
        v = -1 if split_errors is None else int(split_errors)
        if self.L.flx_adapters_set_split(self.h, v) != _lib.FLX_OK:
            raise FlxError(1, "flx_adapters_set_split: split_errors 0..40, or None")
        self.split_errors = None if v < 0 else v

    def __len__(self):
        """the number of patterns: two per sequence"""
        return int(self.L.flx_adapters_patterns(self.h))

    def close(self):
        if self.h:
            self.L.flx_adapters_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _add_seqs(ctx, fn, handle, seqs):
    """The sequences, packed back to back, into the set `handle` through one of the library's add calls."""
    seqs = [bytes(s) for s in seqs]
    n = len(seqs)
    lengths = np.array([len(s) for s in seqs], dtype=np.int64)
    offsets = np.zeros(max(n, 1), dtype=np.uint64)
    if n:
        offsets[1:n] = np.cumsum(lengths[:-1])
    bases = np.frombuffer(b"".join(seqs) or b"\0", dtype=np.uint8)
    ctx._check(fn(handle, bases.ctypes.data, offsets.ctypes.data, lengths.ctypes.data, n))


class Kmers:
    """Reference 16-mer set on the device — mirrors the reference's Kmers (src/kmers.h:28-56)."""

    def __init__(self, ctx):
        self.ctx = ctx
        h = C.c_void_p()
        ctx._check(ctx.L.flx_kmerset_create(ctx.h, C.byref(h)))
        self.h = h
        self._final = False
        ctx._sets.append(weakref.ref(self))

    def add_assembly_fasta(self, seqs):
        """Kmers::add_assembly_fasta (src/kmers.cpp:61-72) on already-parsed contig sequences."""
        _add_seqs(self.ctx, self.ctx.L.flx_kmerset_add_assembly, self.h, seqs)

    def add_screen_fasta(self, seqs):
        """flx_screen_set_add: the sequences of a contaminant for the screen — cut at every byte outside ACGTacgt, pieces of at
        least 16 bases only, so that an N run puts no poly-A into the set."""
        _add_seqs(self.ctx, self.ctx.L.flx_screen_set_add, self.h, seqs)

    def add_read_fastqs(self, files_of_seqs):
        """Kmers::add_read_fastqs (src/kmers.cpp:50-58): one list of read sequences per file, -1 then -2."""
        for seqs in files_of_seqs:
            _add_seqs(self.ctx, self.ctx.L.flx_kmerset_add_short_reads, self.h, seqs)

    def finalize(self):
        self.ctx._check(self.ctx.L.flx_kmerset_finalize(self.h))
        self._final = True

    def __len__(self):
        return int(self.ctx.L.flx_kmerset_size(self.h))

    def empty(self):
        return len(self) == 0

    def is_kmer_present(self, kmers):
        k = np.ascontiguousarray(kmers, dtype=np.uint32)
        out = np.zeros(len(k), dtype=np.uint8)
        self.ctx._check(self.ctx.L.flx_kmerset_contains(self.h, k.ctypes.data, len(k), out.ctypes.data))
        return out.astype(bool)

    def close(self):
        if self.h:
            if self.ctx.h:  # a set never outlives its context (Context.close() closes its sets first)
                self.ctx.L.flx_kmerset_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ScreenSet:
    """flx_screenset: the canonical K-mers (16 <= K <= 31) of a contaminant as a hash table on the device — what lets the screen
    take a genome.  log2_capacity: the table's first size in slots (None: 2^16); it grows as sequences are added."""

    def __init__(self, ctx, k, log2_capacity=None):
        self.ctx = ctx
        h = C.c_void_p()
        ctx._check(ctx.L.flx_screenset_create(ctx.h, int(k), 16 if log2_capacity is None else int(log2_capacity), C.byref(h)))
        self.h = h
        ctx._sets.append(weakref.ref(self))

    def add_fasta(self, seqs):
        """flx_screenset_add: the sequences as they are; a window with a byte outside ACGTacgt is in no set."""
        _add_seqs(self.ctx, self.ctx.L.flx_screenset_add, self.h, seqs)

    def finalize(self):
        self.ctx._check(self.ctx.L.flx_screenset_finalize(self.h))

    def __len__(self):
        return int(self.ctx.L.flx_screenset_size(self.h))

    @property
    def k(self):
        return int(self.ctx.L.flx_screenset_k(self.h))

    @property
    def capacity(self):
        return int(self.ctx.L.flx_screenset_capacity(self.h))

    def close(self):
        if self.h:
            if self.ctx.h:  # (Context.close() closes its sets first)
                self.ctx.L.flx_screenset_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
