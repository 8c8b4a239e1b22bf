"""GPU tests (-m gpu) of a library job over groups of videos (needle_hip_library_set_groups, include/needle_hip.h), one rank.

The oracle is the checker: a video's expected result is O.run_with_frame_hashes over its own season's sub-list, in list
order; a video alone in its season has none.  The library is tests/library_groups_worker.py's: eight episodes, labels
[5, 9, 5, 7, 9, 5, 3, 9], every episode with the same intro -- the oracle over two videos of DIFFERENT seasons finds it, so
the labels, not the audio, keep the seasons apart.

The run list: the comparator call does not hand its run list out, so the expected list of a grouped job is built from the
PLAIN library's job over the same PCM (the scan of a pair does not depend on which other pairs are scanned): its runs of
same-season pairs, renumbered with needle_hip_group_pairs.  The grouped job's list must equal it run for run, problem ids
included, and needle_hip_comparator_results_from_runs_grouped over it, and Comparator.run_with_frame_hashes(groups=...)
over the library's own frame hashes, must both give the per-season oracle's results."""
import numpy as np
import pytest

from needle_amd import capi, synth
from oracle import oracle as O
from tests import library_groups_worker as W

pytestmark = pytest.mark.gpu
NS = O.NS
LABELS = W.LABELS
FIELDS = ("problem", "src_end", "dst_end", "len", "src_match_hash", "dst_match_hash")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert capi.device_count() > 0, "GPU tests need a HIP device (the product has no CPU fallback)"


def _as(rs):
    return [None if r is None else [None if r.opening is None else list(r.opening),
                                    None if r.ending is None else list(r.ending)] for r in rs]


def _per_season(ocmp, ref, labels):
    """The per-season oracle: every season's own sub-list, in list order."""
    want = [None] * len(labels)
    for members in W.members_of(labels).values():
        if len(members) < 2:
            continue
        for v, r in zip(members, O.run_with_frame_hashes(ocmp, [ref[v] for v in members])):
            want[v] = r
    return _as(want)


def _sorted_runs(runs):
    keys = np.stack([runs[f].astype(np.uint32) for f in FIELDS], axis=1) if len(runs) else np.zeros((0, 6), np.uint32)
    return sorted(map(tuple, keys.tolist()))


def _grouped_from_plain(plain_runs, labels, regions=1):
    """The plain job's runs of same-season pairs under their grouped ids."""
    n = len(labels)
    plain_pairs = [(i, j) for i in range(n) for j in range(i + 1, n)]
    grouped_id = {(int(a), int(b)): p for p, (a, b) in enumerate(capi.group_pairs(labels).tolist())}
    out = []
    for r in _sorted_runs(plain_runs):
        pair = plain_pairs[r[0] // regions]
        if pair in grouped_id:
            out.append((grouped_id[pair] * regions + r[0] % regions,) + r[1:])
    return sorted(out)


@pytest.fixture(scope="module")
def seasons():
    """The eight episodes, the oracle's hashes and per-season results, and the plain library's run list -- made once."""
    eps = [W.episode(k) for k in range(8)]
    hd = O.duration_from_secs_f32(0.3)
    ref = O.analyze_batch([e.pcm[: len(e.pcm) // 2] for e in eps], 1, hd)
    ocmp = O.Comparator(min_opening_duration=10 * NS)
    want = _per_season(ocmp, ref, LABELS)
    # the labels keep the seasons apart, not the audio: a video of season 5 and one of season 9 match, and so does a lone video
    assert all(r is not None and r.opening is not None for r in O.run_with_frame_hashes(ocmp, [ref[0], ref[1]]))
    assert all(r is not None and r.opening is not None for r in O.run_with_frame_hashes(ocmp, [ref[3], ref[4]]))
    assert all(want[v] is not None and want[v][0] is not None for v in (0, 1, 2, 4, 5, 7))
    assert want[3] is None and want[6] is None
    cmp = W.comparator()
    plain = capi.Library(8)
    plain.set_pcm([e.pcm for e in eps], [len(e.pcm) for e in eps])
    plain.job_begin(cmp, 0)
    plain.job_end(cmp, 0)
    plain_runs = plain.job_runs(0)
    expected_runs = _grouped_from_plain(plain_runs, LABELS)
    assert len(expected_runs) >= 6 and len(expected_runs) < len(plain_runs), "the plain job also finds cross-season runs"
    return {"eps": eps, "ref": ref, "want": want, "runs": expected_runs, "cmp": cmp}


def _grouped_library(eps, labels=LABELS):
    lib = capi.Library(len(eps)).set_groups(labels)
    lib.set_pcm([e.pcm for e in eps], [len(e.pcm) for e in eps])
    return lib


@pytest.mark.parametrize("setting", ["default", "host-epilogue", "device-epilogue", "slab-of-4-runs"])
def test_grouped_job_equals_the_per_season_oracle(seasons, monkeypatch, setting):
    """Two jobs in flight, three jobs in all, under each form of the epilogue and through the overflow -> grow -> rescan path."""
    if setting == "host-epilogue":
        monkeypatch.setenv("NEEDLE_HIP_DEVICE_EPILOGUE", "0")
    if setting == "device-epilogue":
        monkeypatch.setenv("NEEDLE_HIP_DEVICE_EPILOGUE", "1")
    if setting == "slab-of-4-runs":
        monkeypatch.setenv("NEEDLE_HIP_SLAB_RUNS", "4")
    eps, want, cmp = seasons["eps"], seasons["want"], seasons["cmp"]
    lib = _grouped_library(eps)
    assert lib.num_pairs() == 6 == len(capi.group_pairs(LABELS)) and lib.groups() == LABELS
    with pytest.raises(capi.NeedleError):
        lib.set_groups([1] * 8)                                  # after set_pcm: refused, the library unchanged
    assert lib.num_pairs() == 6 and lib.groups() == LABELS
    lib.job_begin(cmp, 0)
    lib.job_begin(cmp, 1)
    r0, k0 = lib.job_end(cmp, 0)
    runs0, form0, comm0 = lib.job_runs(0), lib.job_form(0), lib.job_comm_bytes(0)
    lib.job_begin(cmp, 0)
    r1, k1 = lib.job_end(cmp, 1)
    r2, k2 = lib.job_end(cmp, 0)
    assert _as(r0) == want and _as(r1) == want and _as(r2) == want
    assert r0[3] is None and r0[6] is None
    assert k0 == k1 == k2 == len(seasons["runs"])
    if setting == "host-epilogue":
        assert form0["device_epilogue"] is False
    if setting == "device-epilogue":
        assert form0["device_epilogue"] is True and lib.job_form(1)["device_epilogue"] is True
    if setting == "slab-of-4-runs":
        # the first two jobs were enqueued with the 4-run slab; the third after it had grown
        assert comm0["scans_repeated"] >= 1 and lib.job_comm_bytes(0)["scans_repeated"] == 0
    for runs in (runs0, lib.job_runs(1), lib.job_runs(0)):
        assert _sorted_runs(runs) == seasons["runs"]              # run for run, problem ids included
        assert all(int(p) < 6 for p in runs["problem"]), "a run of a pair that is no same-season pair"
    # the host half of the grouped comparator call over this list, and the whole grouped call over the library's own hashes
    fhs = [lib.frame_hashes(v) for v in range(8)]
    for v in range(8):
        assert fhs[v].opening_data()[0].tolist() == [h for h, _ in seasons["ref"][v].opening]
    assert _as(cmp.results_from_runs_grouped(fhs, LABELS, runs0)) == want
    assert _as(cmp.run_with_frame_hashes(fhs, groups=LABELS)) == want
    assert _as(lib.finalize(cmp, runs0)) == want


def test_search_ranges_of_grouped_pair_ids_give_the_jobs_run_list(seasons):
    """needle_hip_library_search over [0, 2) and [2, 4) and [4, 6) of the six grouped pairs: together the job's run list."""
    eps, cmp = seasons["eps"], seasons["cmp"]
    lib = _grouped_library(eps)
    lib.analyze()
    capacity = 1024
    d_runs, d_count = capi.DeviceBuffer(capacity * capi.RUN_DTYPE.itemsize), capi.DeviceBuffer(4)
    got = []
    for first, count in ((0, 2), (2, 2), (4, 2)):
        lib.search(cmp, first, count, d_runs.ptr, capacity, d_count.ptr, sync=True)
        total = int(d_count.to_host(np.uint32, 1)[0])
        assert 0 < total <= capacity
        runs = d_runs.to_host(capi.RUN_DTYPE, total)
        assert all(first <= int(p) < first + count for p in runs["problem"])
        got += _sorted_runs(runs)
    with pytest.raises(capi.NeedleError):
        lib.search(cmp, 5, 2, d_runs.ptr, capacity, d_count.ptr, sync=True)      # beyond the grouped pairs
    assert sorted(got) == seasons["runs"]


def test_one_label_for_all_is_the_plain_library_byte_for_byte(monkeypatch):
    lib7 = synth.make_library(7, 90.0, 20.0)
    cmp = W.comparator(7)
    pcm, lens = [e.pcm for e in lib7], [len(e.pcm) for e in lib7]
    for epilogue in ("0", "1"):
        monkeypatch.setenv("NEEDLE_HIP_DEVICE_EPILOGUE", epilogue)
        plain, grouped = capi.Library(7), capi.Library(7).set_groups([77] * 7)
        got = []
        for lib in (plain, grouped):
            lib.set_pcm(pcm, lens)
            lib.job_begin(cmp, 0)
            res, found = lib.job_end(cmp, 0)
            assert lib.job_form(0)["device_epilogue"] is (epilogue == "1")
            got.append((_as(res), found, _sorted_runs(lib.job_runs(0))))
        assert plain.num_pairs() == grouped.num_pairs() == 21
        assert got[0] == got[1] and got[0][1] >= 21 and all(r is not None for r in got[0][0])


def test_every_video_alone_scans_nothing(seasons, monkeypatch):
    eps, cmp = seasons["eps"], seasons["cmp"]
    # a scan of another object first, so that "the last launch" is a known one
    other = capi.Library(3)
    other.set_pcm([e.pcm for e in eps[:3]], [len(e.pcm) for e in eps[:3]])
    other.job_begin(W.comparator(3), 0)
    other.job_end(W.comparator(3), 0)
    try:
        for epilogue in (None, "1"):                              # the device form refuses a job without pairs: the host form takes it
            if epilogue:
                monkeypatch.setenv("NEEDLE_HIP_DEVICE_EPILOGUE", epilogue)
            before = capi.scan_last_launch()
            capi.set_kernel_timing("all,sum")                     # (launch counts start here)
            lib = _grouped_library(eps, list(range(100, 108)))
            assert lib.num_pairs() == 0
            lib.job_begin(cmp, 0)
            lib.job_begin(cmp, 1)
            for slot in (0, 1):
                res, found = lib.job_end(cmp, slot)
                assert res == [None] * 8 and found == 0 and len(lib.job_runs(slot)) == 0
                assert lib.job_form(slot)["device_epilogue"] is False
            assert capi.scan_last_launch() == before
            for name in ("hamming_runs", "hamming_runs_unstaged", "simhash_runs", "epilogue_buckets", "epilogue_entries", "epilogue_best_match"):
                assert capi.kernel_launches(name) == 0, name
            assert lib.finalize(cmp, np.zeros(0, dtype=capi.RUN_DTYPE)) == [None] * 8
    finally:
        capi.set_kernel_timing(None)


def _ending_oracle(eps, hd):
    ref = []
    for e in eps:
        dur = O.duration_from_secs_f64(len(e.pcm) * (1.0 / 11025.0))
        n_open = O.duration_mul_f32(dur, 0.5) * 11025 // NS
        seek = O.duration_mul_f32(dur, float(np.float32(1.0) - np.float32(0.25)))
        first = seek * 11025 // NS
        op = O.step_and_timestamp(O.fingerprint(e.pcm[:n_open]), hd)
        en = O.step_and_timestamp(O.fingerprint(e.pcm[first:]), hd, seek_to_ns=seek)
        ref.append(O.FrameHashes(op, en, hd, ""))
    return ref


@pytest.mark.parametrize("epilogue", ["0", "1"])
def test_endings_ragged_lengths_and_a_video_without_ending_data(monkeypatch, epilogue):
    """Two regions per pair, episodes of 100 .. 135 s with an intro and an outro, and one video of 8 s whose ending window
    keeps no hash: alone in its season it is nobody's partner and the job succeeds; inside a season the job fails as the
    reference does."""
    monkeypatch.setenv("NEEDLE_HIP_DEVICE_EPILOGUE", epilogue)
    eps = [synth.make_episode(k, 100.0 + 7.0 * k, 22.0, 21.0) for k in range(6)]
    short = synth.make_episode(6, 8.0, 2.0)
    eps.insert(3, short)                                         # positions: 0 1 2 [short] 3 4 5
    labels = [1, 2, 1, 6, 2, 1, 2]
    hd = O.duration_from_secs_f32(0.3)
    ocmp = O.Comparator(include_endings=True, min_opening_duration=10 * NS, min_ending_duration=10 * NS)
    ref = _ending_oracle([e for k, e in enumerate(eps) if k != 3], hd)
    ref.insert(3, None)                                          # (never handed to the oracle: it has no pair)
    want = _per_season(ocmp, ref, labels)
    assert want[3] is None and all(want[v] is not None and want[v][0] is not None and want[v][1] is not None for v in (0, 1, 2, 4, 5, 6))
    cmp = capi.Comparator([f"ep{k}.wav" for k in range(7)], min_opening_duration=10, min_ending_duration=10, include_endings=True)
    lib = capi.Library(7).include_endings().set_groups(labels)
    lib.set_pcm([e.pcm for e in eps], [len(e.pcm) for e in eps])
    lib.job_begin(cmp, 0)
    res, found = lib.job_end(cmp, 0)
    assert lib.frame_hashes(3).ending_data()[0].size == 0 and lib.frame_hashes(3).opening_data()[0].size > 0
    assert _as(res) == want and found >= 12
    assert lib.job_form(0)["device_epilogue"] is (epilogue == "1")
    runs = lib.job_runs(0)
    assert {int(p) % 2 for p in runs["problem"]} == {0, 1} and all(int(p) < 12 for p in runs["problem"])
    fhs = [lib.frame_hashes(v) for v in range(7)]
    assert _as(cmp.results_from_runs_grouped(fhs, labels, runs)) == want
    # the same video inside a season
    inside = capi.Library(7).include_endings().set_groups([1, 2, 1, 2, 2, 1, 2])
    inside.set_pcm([e.pcm for e in eps], [len(e.pcm) for e in eps])
    with pytest.raises(capi.NeedleError, match="no ending hash data present"):
        inside.job_begin(cmp, 0)
        inside.job_end(cmp, 0)
