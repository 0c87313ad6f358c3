"""Every record of full-size list-decoder launches against the CPU oracle.

The suite's other full-size tests check properties and self-consistency (pipeline == decode_batch, fused == unfused, ...):
a systematic kernel error passes them.  These compare EVERY record with the oracle, at the sizes where the lane-per-path
list decoder (es_scl_wide.hip) reuses its scratch-slab slots many times over and draws frames from its counter for long:

  * test_headline_step_every_record_vs_oracle: bench.py's config-3 step (65 536 device-made windows, three lanes in
    flight together), every stage of every record -- sync, LLR, hard decision, compaction, list, selection;
  * test_list_decoder_device_filling_launches_vs_oracle: the list decoder alone at L = 1 .. 32, at least three times as
    many blocks as the slab has slots, distinct rows that mostly reach the list loop, both skip modes and both mappings.

The oracle runs on a thread pool (oracle.map_records); workers compare and return only mismatch descriptors
(record, field, first differing index)."""
import time
from collections import Counter

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from echoseal_amd.tables import pack_tables

KEY = b"\xAA" * 32
B3 = 65536                      # bench.py --windows default: the headline step's records


def _report(mism, what):
    if mism:
        by = Counter(f for _, f, _ in mism)
        recs = sorted({r for r, _, _ in mism})
        raise AssertionError(f"{what}: {len(mism)} mismatches in {len(recs)} records; by field {dict(by)}; "
                             f"first records {recs[:12]}; first descriptors {mism[:12]}")


def _slab_slots(dev) -> int:
    """Slots of the lane-per-path list decoder's scratch slab for one-wave (64-lane) blocks, list_size_max <= 64:
    num_cu x WIDE_WPS (3, waves per SIMD the kernel is built for) x 4 (es_scl_wide_scratch_bytes sizes the slab in
    256-lane blocks; launch_wide cuts each into four 64-lane slots)."""
    return torch.cuda.get_device_properties(dev).multi_processor_count * 3 * 4


def test_headline_step_every_record_vs_oracle(oracle):
    """bench.py's config-3 step, built as bench.py builds it: device schedule, device-made frames and windows (seed 34),
    an 8-list DecodePipeline of three lanes (one lane per path by launch size, slab slots, frame counter), fused sync,
    LLR at the first detected peak, compacted list decoder, on-device selection.  The same step on all three lanes back to
    back (launches in flight together, as the benchmark's rotating steps are) gives identical outputs, and every record
    equals the oracle bit for bit."""
    from echoseal_amd import workloads as WL
    from echoseal_amd.embedder import WatermarkEmbedder
    from echoseal_amd.engine import DecodePipeline, RxEngine
    t0 = time.perf_counter()
    eng = RxEngine(0, list_size_max=16)
    dev = eng.device
    tx = WatermarkEmbedder(KEY)
    pn, band = eng.schedule(tx.sec._prng.sub_key, KEY, ctr0=0, n=B3)
    clean = torch.cat([eng.synthetic_frames(KEY, c0, 16384)[0] for c0 in range(0, B3, 16384)])
    win, _off = WL.c3_windows_device(clean, seed=34)
    del clean
    pipe = DecodePipeline(eng, list_size=8, lanes=3)
    for e in pipe.lane_engs:
        e.set_option("scl_multi", -1); e.set_option("scl_lane_slab", 1)
    outs = [pipe.submit(win, band, pn, start="peak", select=True) for _ in range(3)]
    torch.cuda.synchronize()
    t_gpu = time.perf_counter() - t0
    # three lanes, one step: identical
    sy0, llr0, scl0, _ = outs[0]
    for j, (sy, llr, scl, _d) in enumerate(outs[1:], 1):
        for name in ("y", "thr", "peaks", "npeaks", "flags"):
            assert torch.equal(getattr(sy, name), getattr(sy0, name)), (j, name)
        assert torch.equal(llr, llr0), (j, "llr")
        for name in ("hard_info", "hard_ok", "ncand", "cand_info", "cand_metric", "cand_ok"):
            assert torch.equal(getattr(scl, name), getattr(scl0, name)), (j, name)
        for k in range(3):
            assert torch.equal(scl.selected[k], scl0.selected[k]), (j, "selected", k)
    # host copies of everything compared (the band-passed signal on a seeded sample)
    rng = np.random.default_rng(34)
    ysel = np.sort(rng.choice(B3, 1024, replace=False))
    ypos = {int(i): k for k, i in enumerate(ysel)}
    ys = sy0.y[torch.from_numpy(ysel).to(dev)].cpu().numpy()
    h = {n: t.cpu().numpy() for n, t in dict(thr=sy0.thr, pk=sy0.peaks, npk=sy0.npeaks, llr=llr0, hinfo=scl0.hard_info,
                                             hok=scl0.hard_ok, nc=scl0.ncand, ci=scl0.cand_info, cm=scl0.cand_metric,
                                             cc=scl0.cand_ok, pay=scl0.selected[0], ok=scl0.selected[1],
                                             which=scl0.selected[2]).items()}
    W = win.cpu().numpy(); P = pn.cpu().numpy(); Bd = band.cpu().numpy().astype(np.int64)
    del outs, sy0, llr0, scl0, win
    pipe.synchronize(); del pipe
    ba, tpl, taps, ntaps, _ = pack_tables()

    def cmp(lo, hi):
        out = []
        for i in range(lo, hi):
            b = Bd[i]
            o = oracle.headline_record(W[i], ba[b], tpl[b], taps[b, :ntaps[b]], np.unpackbits(P[i])[:1215], L=8)

            def chk(field, want, got):
                d = oracle.first_diff(want, got)
                if d is not None:
                    out.append((i, field, d))
            chk("thr", np.float64(o["thr"]), h["thr"][i])
            k = int(h["npk"][i]) & 0xFFFF
            if k != min(o["npeaks"], 32):
                out.append((i, "npeaks", k))
            if bool((int(h["npk"][i]) >> 30) & 1) != o["fallback"]:
                out.append((i, "fallback", 0))
            chk("peaks", o["peaks"][:k].astype(np.int32), h["pk"][i, :k])
            if i in ypos:
                chk("y", o["y"], ys[ypos[i]])
            chk("llr", o["llr"], h["llr"][i])
            chk("hard_info", o["hard_info"], h["hinfo"][i])
            if int(h["hok"][i]) != int(o["hard_ok"]):
                out.append((i, "hard_ok", int(h["hok"][i])))
            if (int(h["nc"][i]) == 0) != o["hard_ok"]:                    # compaction: no list exactly when the hard decision passes
                out.append((i, "compaction", int(h["nc"][i])))
            elif int(h["nc"][i]) != o["ncand"]:
                out.append((i, "ncand", int(h["nc"][i])))
            chk("cand_info", o["cand_info"], h["ci"][i])
            chk("cand_metric", o["cand_metric"], h["cm"][i])
            chk("cand_ok", o["cand_ok"], h["cc"][i])
            chk("payload", o["payload"], h["pay"][i])
            if int(h["ok"][i]) != o["ok"] or int(h["which"][i]) != o["which"]:
                out.append((i, "selected", (int(h["ok"][i]), int(h["which"][i]))))
        return out
    t1 = time.perf_counter()
    mism = oracle.map_records(cmp, B3, chunk=256)
    t_oracle = time.perf_counter() - t1
    listed = int((h["nc"] > 0).sum()); crc_ok = int((h["ok"] == 1).sum())
    print(f"\nheadline step: {B3} records, listed {listed} ({listed / B3:.4f}), selected ok == 1: {crc_ok}, "
          f"ok != 1: {B3 - crc_ok}, fallback {int(((h['npk'] >> 30) & 1).sum())}; GPU part {t_gpu:.1f} s, "
          f"oracle {t_oracle:.1f} s on {oracle.map_threads()} threads")
    _report(mism, "headline step vs oracle")
    assert listed > 0.9 * B3                                # the list decoder is what this test exercises
    assert 0 < crc_ok < B3


def _rows(eng, L, B):
    """B distinct LLR rows [B, 1024] float32 (every value exact in float32, so the float64 launch sees the same numbers), made
    on the device from seeded random codewords: 10/16 noisy at five noise levels, 2/16 clean, 2/16 clipped at +-12,
    2/16 small integers with some signs flipped (exact metric ties)."""
    dev = eng.device
    g = torch.Generator(device=dev); g.manual_seed(7000 + L)
    info = torch.randint(0, 256, (B, 55), dtype=torch.uint8, device=dev, generator=g)
    s = eng.polar_encode(info).to(torch.float32) * 2 - 1                       # +1 for a one bit (positive LLR = 1)
    kind = torch.arange(B, device=dev) % 16
    sigma = torch.tensor([0.45, 0.55, 0.65, 0.75, 0.9], device=dev)[kind % 5][:, None]
    noisy = 2 * (s + sigma * torch.randn((B, 1024), device=dev, generator=g)) / (sigma * sigma)
    clipped = (4 * noisy).clamp(-12, 12)
    ints = torch.randint(1, 4, (B, 1024), device=dev, generator=g).to(torch.float32)
    flip = torch.where(torch.rand((B, 1024), device=dev, generator=g) < 0.12, -1.0, 1.0)
    ties = s * ints * flip
    k = kind[:, None]
    x = torch.where(k < 10, noisy, torch.where(k < 12, 3.0 * s, torch.where(k < 14, clipped, ties)))
    return x.to(torch.float32).contiguous()


@pytest.fixture(scope="module")
def wide_engine():
    from echoseal_amd.engine import RxEngine
    eng = RxEngine(0, list_size_max=32)
    eng.set_option("scl_lane_slab", 1)
    yield eng
    eng.close()


@pytest.mark.parametrize("L", [1, 2, 4, 8, 16, 32])
def test_list_decoder_device_filling_launches_vs_oracle(wide_engine, oracle, L):
    """The list decoder at launch sizes where the lane-per-path kernel's blocks outnumber its slab's slots at least three to
    one (slot release and reuse across XCDs, frames drawn from the counter for long), L = 1 capped at 131 072 rows:
    forced one lane per path (scl_multi 1, scl_lanes 1) and the library's own choice (scl_multi -1), float32 and float64
    LLRs, skip_if_hard_ok on and off.  Runs of one skip mode are identical; every row equals the oracle bit for bit."""
    eng = wide_engine
    frames_per_block = 64 // L                                   # one-wave blocks, 64 / L frames each
    B = 3 * _slab_slots(eng.device) * frames_per_block
    if L == 1:
        B = min(B, 131072)
    t0 = time.perf_counter()
    x32 = _rows(eng, L, B)
    x64 = x32.to(torch.float64)
    runs = {}
    for mapping in ("lane_per_path", "auto"):
        if mapping == "lane_per_path":
            eng.set_option("scl_multi", 1); eng.set_option("scl_lanes", 1)
        else:
            eng.set_option("scl_multi", -1); eng.set_option("scl_lanes", 0)
        for x in (x32, x64):
            for skip in (False, True):
                runs[(mapping, x.dtype, skip)] = eng.scl(x, list_size=L, skip_if_hard_ok=skip).check()
    eng.set_option("scl_multi", -1); eng.set_option("scl_lanes", 0)
    torch.cuda.synchronize()
    names = ("hard_info", "hard_ok", "ncand", "cand_info", "cand_metric", "cand_ok")
    ref = {skip: runs[("lane_per_path", torch.float32, skip)] for skip in (False, True)}
    for (mapping, dt, skip), r in runs.items():
        for n in names:
            assert torch.equal(getattr(r, n), getattr(ref[skip], n)), (mapping, dt, skip, n)
    for n in ("hard_info", "hard_ok"):
        assert torch.equal(getattr(ref[True], n), getattr(ref[False], n)), n
    X = x32.cpu().numpy()
    F = {n: getattr(ref[False], n).cpu().numpy() for n in names}
    S = {n: getattr(ref[True], n).cpu().numpy() for n in ("ncand", "cand_info", "cand_metric", "cand_ok")}
    del runs, ref, x32, x64
    t_gpu = time.perf_counter() - t0

    def cmp(lo, hi):
        out = []
        for i in range(lo, hi):
            llr = X[i].astype(np.float64)

            def chk(field, want, got):
                d = oracle.first_diff(want, got)
                if d is not None:
                    out.append((i, field, d))
            hinfo, hok = oracle.polar_hard(llr)
            chk("hard_info", np.packbits(hinfo), F["hard_info"][i])
            if int(F["hard_ok"][i]) != int(hok):
                out.append((i, "hard_ok", int(F["hard_ok"][i])))
            nn, ci, cm, cc = oracle.scl_list(llr, L)
            ci = np.packbits(ci, axis=1)
            if int(F["ncand"][i]) != nn:
                out.append((i, "ncand", int(F["ncand"][i])))
            chk("cand_info", ci, F["cand_info"][i])
            chk("cand_metric", cm, F["cand_metric"][i])
            chk("cand_ok", cc, F["cand_ok"][i])
            if hok:                                              # skipped: no list, zero rows
                if int(S["ncand"][i]) != 0:
                    out.append((i, "skip/compaction", int(S["ncand"][i])))
                ci, cm, cc = np.zeros_like(ci), np.zeros_like(cm), np.zeros_like(cc)
            elif int(S["ncand"][i]) != nn:
                out.append((i, "skip/ncand", int(S["ncand"][i])))
            chk("skip/cand_info", ci, S["cand_info"][i])
            chk("skip/cand_metric", cm, S["cand_metric"][i])
            chk("skip/cand_ok", cc, S["cand_ok"][i])
        return out
    t1 = time.perf_counter()
    mism = oracle.map_records(cmp, B, chunk=max(16, 4096 // L))
    t_oracle = time.perf_counter() - t1
    n_ok = int(F["hard_ok"].sum())
    print(f"\nL={L}: {B} rows ({B // frames_per_block} blocks, {_slab_slots(eng.device)} slots), hard decision passes "
          f"{n_ok}; GPU part {t_gpu:.1f} s, oracle {t_oracle:.1f} s on {oracle.map_threads()} threads")
    _report(mism, f"L = {L}, {B} rows vs oracle")
    assert 0.05 * B < n_ok < 0.7 * B                             # both skip branches are taken, most rows reach the list loop
