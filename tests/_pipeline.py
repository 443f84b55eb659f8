"""End-to-end composition of the hot path the way the reference's main() composes it
(src/main.cpp:63-313), parametrised by backend so the SAME driver checks the CPU oracle (here) and
the HIP library (on the GPU box) against the golden outputs of the real reference binary.

TEST INFRASTRUCTURE.  The product's host side is the C++ CLI; this file only exists so that parity
tests read like the reference's own black-box tests (ordered output names, child coordinates,
summary numbers).
"""
import numpy as np

import _oracle


class OracleBackend:
    name = "oracle"

    def kmers(self, assembly=None, short_files=None):
        if assembly is None and not short_files:
            return None
        ks = _oracle.KmerSet()
        if assembly is not None:
            ks.add_assembly(assembly)
        for f in (short_files or []):
            ks.add_short_reads(f)
        return ks

    def kmers_empty(self, ks):
        return ks is None or len(ks) == 0

    def score(self, reads, pkw, ks, split_window_q=None):
        p = _oracle.make_params(**pkw)
        kmer_mode = not self.kmers_empty(ks)
        res = []
        for name, seq, qual in reads:
            o = _oracle.score_read(seq, qual if qual is not None else b"\0" * len(seq), p, ks if kmer_mode else None)
            res.append(o)
        if split_window_q is not None:
            # --split_window_q (Phred mode): the children are the model's, each scored as a read of its own on its quality substring;
            # the parents keep their scores and a wholly bad read fails
            import _qsplit_model as model
            assert not kmer_mode
            off, rng, first, last, wholly = model.split_batch([qual for _, _, qual in reads], pkw.get("window_size", 250), split_window_q)
            for i, ((name, seq, qual), o) in enumerate(zip(reads, res)):
                ranges = [(int(s), int(e)) for s, e in rng[int(off[i]):int(off[i + 1])]]
                kids = [_oracle.score_read(None, qual[s:e], p) for s, e in ranges]
                o.update(first=int(first[i]), last=int(last[i]), child_ranges=ranges, passed=0 if wholly[i] else o["passed"],
                         children=[{k: c[k] for k in ("length", "mean_q", "window_q", "passed")} for c in kids])
        return res

    def reads2(self, lengths, sc):
        return _oracle.reads2_gather(lengths, sc)

    def rank(self, mean_q, window_q, length, passed, **kw):
        r = _oracle.rank_and_cut(mean_q, window_q, length, passed, **kw)
        return r["passed"], r["target_bases"], r["kept_bases"], r["outcome"]


class HipBackend:
    name = "hip"

    def __init__(self, ctx=None):
        from filtlong_amd import api
        self.api = api
        self.ctx = ctx or api.Context(0)

    def kmers(self, assembly=None, short_files=None):
        if assembly is None and not short_files:
            return None
        ks = self.api.Kmers(self.ctx)
        if assembly is not None:
            ks.add_assembly_fasta(assembly)
        if short_files:
            ks.add_read_fastqs(short_files)
        ks.finalize()
        return ks

    def kmers_empty(self, ks):
        return ks is None or ks.empty()

    def score(self, reads, pkw, ks, split_window_q=None):
        api = self.api
        p = api.make_params(**pkw)
        kmer_mode = not self.kmers_empty(ks)
        strings = [(seq if kmer_mode else qual) for _, seq, qual in reads]
        plane, offsets, lengths = api.pack_reads(strings)
        order = api.length_order(lengths)
        o = self.ctx.score_reads(plane, offsets, lengths, p, kmers=ks if kmer_mode else None, order=order, split_window_q=split_window_q)
        res = []
        co = o["child_offsets"]
        for i in range(len(reads)):
            a, b = int(co[i]), int(co[i + 1])
            res.append({
                "length": int(lengths[i]), "mean_q": float(o["mean_q"][i]), "window_q": float(o["window_q"][i]),
                "passed": int(o["passed"][i]), "first": int(o["first"][i]), "last": int(o["last"][i]),
                "child_ranges": [tuple(int(x) for x in r) for r in o["child_ranges"][a:b]],
                "children": [{"length": int(o["child_ranges"][j][1] - o["child_ranges"][j][0]),
                              "mean_q": float(o["child_mean_q"][j]), "window_q": float(o["child_window_q"][j]),
                              "passed": int(o["child_passed"][j])} for j in range(a, b)],
            })
        return res

    def reads2(self, lengths, sc):
        return self.ctx.reads2_gather(lengths, sc)

    def rank(self, mean_q, window_q, length, passed, lw=1.0, mw=1.0, ww=1.0, **kw):
        r = self.ctx.rank_and_cut(mean_q, window_q, length, passed, length_weight=lw, mean_q_weight=mw,
                                  window_q_weight=ww, **kw)
        rep = r["report"]
        self.last_report = rep
        return r["passed"], rep.target_bases, rep.kept_bases, rep.outcome


class SplitWindowQ:
    """A backend whose scoring call splits at low-quality windows (--split_window_q q); everything else is the backend's own."""

    def __init__(self, backend, q):
        self.backend, self.q = backend, q

    def __getattr__(self, name):
        return getattr(self.backend, name)

    def score(self, reads, pkw, ks):
        return self.backend.score(reads, pkw, ks, split_window_q=self.q)


def run_filter(backend, reads, ks, pkw=None, target_bases=None, keep_percent=None, lw=1.0, mw=1.0, ww=1.0):
    """Returns (ordered output names, after_count, after_bases, target, kept, outcome) like the reference CLI."""
    pkw = pkw or {}
    scored = backend.score(reads, pkw, ks)
    # reads2 gather, main.cpp:138-147, through the backend's seam (oracle: flo_reads2_gather, HIP: flx_reads2_gather);
    # child names read.cpp:135-136
    lengths = np.array([len(seq) for _, seq, _ in reads], dtype=np.int32)
    kids = [c for r in scored for c in r["children"]]
    rngs = [x for r in scored for x in r["child_ranges"]]
    sc = {"mean_q": np.array([r["mean_q"] for r in scored], dtype=np.float64),
          "window_q": np.array([r["window_q"] for r in scored], dtype=np.float64),
          "passed": np.array([r["passed"] for r in scored], dtype=np.uint8),
          "child_offsets": np.concatenate([[0], np.cumsum([len(r["children"]) for r in scored])]).astype(np.uint64),
          "child_ranges": np.array(rngs, dtype=np.int32).reshape(-1, 2),
          "child_mean_q": np.array([c["mean_q"] for c in kids], dtype=np.float64),
          "child_window_q": np.array([c["window_q"] for c in kids], dtype=np.float64),
          "child_passed": np.array([c["passed"] for c in kids], dtype=np.uint8)}
    r2 = backend.reads2(lengths, sc)
    names = []
    for par, ch in zip(r2["parent"], r2["child"]):
        if ch < 0:
            names.append(reads[par][0])
        else:
            names.append("%s_%d-%d" % (reads[par][0], rngs[ch][0] + 1, rngs[ch][1]))
    mean_q, window_q, length, passed = r2["mean_q"], r2["window_q"], r2["length"], r2["passed"]
    total_bases = sum(len(seq) for _, seq, _ in reads)  # original reads, main.cpp:89
    out_passed, target, kept, outcome = backend.rank(
        np.array(mean_q), np.array(window_q), np.array(length, dtype=np.int32), np.array(passed, dtype=np.uint8),
        lw=lw, mw=mw, ww=ww, target_bases=target_bases, keep_percent=keep_percent, total_bases=total_bases)
    out_names = [n for n, p in zip(names, out_passed) if p]
    return out_names, len(names), int(np.asarray(length, dtype=np.int64).sum()), int(target), int(kept), int(outcome)


def golden_args_to_kwargs(args):
    """Parse the filtlong argv stored in tests/golden/e2e.json into run_filter keyword arguments."""
    pkw, kw, ref = {}, {}, {}
    i = 0
    while i < len(args):
        a = args[i]
        v = args[i + 1] if i + 1 < len(args) else None
        if a == "--target_bases": kw["target_bases"] = int(v); i += 2
        elif a == "--keep_percent": kw["keep_percent"] = float(v); i += 2
        elif a == "--min_length": pkw["min_length"] = int(v); i += 2
        elif a == "--max_length": pkw["max_length"] = int(v); i += 2
        elif a == "--min_mean_q": pkw["min_mean_q"] = float(v); i += 2
        elif a == "--min_window_q": pkw["min_window_q"] = float(v); i += 2
        elif a == "--window_size": pkw["window_size"] = int(v); i += 2
        elif a == "--split": pkw["split"] = int(v); i += 2
        elif a == "--trim": pkw["trim"] = True; i += 1
        elif a == "--length_weight": kw["lw"] = float(v); i += 2
        elif a == "--mean_q_weight": kw["mw"] = float(v); i += 2
        elif a == "--window_q_weight": kw["ww"] = float(v); i += 2
        elif a == "-a": ref["a"] = v; i += 2
        elif a == "-1": ref["1"] = v; i += 2
        elif a == "-2": ref["2"] = v; i += 2
        else: raise ValueError(a)
    return pkw, kw, ref
