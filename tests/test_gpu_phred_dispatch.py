"""The Phred dispatch without a wait in front of the kernel (score_phred_regs.hip): the table variant is chosen on the device, the
kernel leaves reads from the long threshold on to the cooperative path.  score_reads_dev with each table variant forced, with
the device's own choice on narrow and wide data, and with reads above the long threshold, against the direct kernel
(FLX_PHRED_KERNEL=direct, one lane per read, byte by byte): every field bit-identical."""
import numpy as np
import pytest

from filtlong_amd import api

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


def batch(seed, n, wide, long_reads=()):
    rng = np.random.default_rng(seed)
    lens = list(np.minimum(rng.gamma(2.0, 1500.0, n).astype(np.int64) + 1, 30_000)) + list(long_reads)
    quals = []
    for i, L in enumerate(lens):
        if wide:  # per-read centre Q3..Q44: entries e and e + 32 of a plain table collide
            q = rng.integers(3, 45) + rng.integers(-3, 4, int(L))
        else:
            q = 15 + rng.integers(-4, 5, int(L))
        quals.append((np.clip(q, 0, 60) + 33).astype(np.uint8).tobytes())
    quals[3] = b""
    r = np.frombuffer(quals[5], dtype=np.uint8).copy()
    r[len(r) // 2] = 200  # a byte >= 128: the bank-private tables hand such a read to the redo kernel
    quals[5] = r.tobytes()
    return quals


def score_dev(ctx, quals, ws):
    import torch
    plane, offsets, lengths = api.pack_reads(quals)
    n = len(quals)
    order = api.length_order(lengths)
    d_plane = torch.from_numpy(plane).cuda()
    d_off = torch.from_numpy(offsets.view(np.int64)).cuda()
    d_len = torch.from_numpy(lengths).cuda()
    d_ord = torch.from_numpy(order.view(np.int32)).cuda()
    mean = torch.full((n,), -1.0, dtype=torch.float64, device="cuda")
    win = torch.full((n,), -1.0, dtype=torch.float64, device="cuda")
    ok = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.timing_enable(True)
    ctx.timing_reset()
    ctx.score_reads_dev(d_plane.data_ptr(), len(plane), d_off.data_ptr(), d_len.data_ptr(), d_ord.data_ptr(), n,
                        api.make_params(window_size=ws, min_length=200, min_window_q=30.0), mean.data_ptr(), win.data_ptr(), ok.data_ptr())
    kernel = ctx.last_phred_kernel()
    timed = ctx.timing_get(kernel)[1]
    long_launches = ctx.timing_get("flx_score_phred_long")[1]
    ctx.timing_enable(False)
    torch.cuda.synchronize()
    return {"mean_q": mean.cpu().numpy(), "window_q": win.cpu().numpy(), "passed": ok.cpu().numpy(), "kernel": kernel,
            "timed": timed, "long": long_launches}


def same(got, want, what):
    for key in ("mean_q", "window_q"):
        g, w = got[key], want[key]
        assert (np.isnan(g) == np.isnan(w)).all(), what + " " + key
        assert ((g.view(np.uint64) == w.view(np.uint64)) | np.isnan(w)).all(), what + " " + key
    assert (got["passed"] == want["passed"]).all(), what + " passed"


@pytest.mark.parametrize("ws", [7, 250, 520])
@pytest.mark.parametrize("wide", [False, True])
def test_table_variants_and_long_reads(ctx, ws, wide, monkeypatch):
    quals = batch(ws + wide, 3000, wide, long_reads=(5000, 70_000))
    monkeypatch.setenv("FLX_PHRED_LONG_MIN", "0")
    monkeypatch.setenv("FLX_PHRED_KERNEL", "direct")
    want = score_dev(ctx, quals, ws)
    assert want["kernel"] == "flx_score_phred_direct"
    monkeypatch.delenv("FLX_PHRED_KERNEL")
    for tables in ("plain", "private", None):
        for long_min in ("0", "40000", "4000"):  # off / one read above the threshold / many
            if tables:
                monkeypatch.setenv("FLX_PHRED_TABLES", tables)
            else:
                monkeypatch.delenv("FLX_PHRED_TABLES", raising=False)
            monkeypatch.setenv("FLX_PHRED_LONG_MIN", long_min)
            got = score_dev(ctx, quals, ws)
            what = "ws=%d wide=%s tables=%s long_min=%s" % (ws, wide, tables, long_min)
            same(got, want, what)
            assert (got["long"] > 0) == (long_min != "0"), what
            # the kernel that did the work is named, and its one timing bracket carries that name
            if ws >= 512 or tables == "plain":
                assert got["kernel"] == "flx_score_phred_regs", what
            elif tables == "private":
                assert got["kernel"] == "flx_score_phred_regs_private", what
            else:
                assert got["kernel"] == ("flx_score_phred_regs_private" if wide else "flx_score_phred_regs"), what
            assert got["timed"] == 1, what


def test_every_read_long(ctx, monkeypatch):
    quals = batch(9, 50, False)
    monkeypatch.setenv("FLX_PHRED_LONG_MIN", "0")
    monkeypatch.setenv("FLX_PHRED_KERNEL", "direct")
    want = score_dev(ctx, quals, 250)
    monkeypatch.delenv("FLX_PHRED_KERNEL")
    monkeypatch.setenv("FLX_PHRED_LONG_MIN", "1")
    got = score_dev(ctx, quals, 250)
    same(got, want, "all long")
    assert got["long"] > 0
