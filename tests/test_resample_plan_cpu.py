"""The resampler's kernel plan of EVERY rate the product accepts, without a GPU: needle_hip_resample_plan answers from the
KernelPlan the launch itself reads (needle_amd/csrc/resample.hip), so a sweep over all 766 001 rates can check each
kernel's own preconditions -- stated here from the kernels' comments, not from the planner's expressions --, count the
classes of plans, and prove that tests/test_gpu_resample_plans.py's rate table (tests/resample_plans.py) holds a rate of
every class.  The sweep takes seconds because a plan evaluates no coefficient."""
import ctypes as C
import time

import numpy as np
import pytest

from needle_amd import capi
from tests import resample_plans as P

FAM = {name: k for k, name in enumerate(capi.RESAMPLE_FAMILIES)}
INVALID = capi.ERROR_NAMES.index("InvalidArgument")
LDS_LIMIT = 160 * 1024            # bytes of LDS a workgroup of the MI355X can have
MAX_REGION_SAMPLES = 30000        # resample.hip, kMaxRegionSamples: f32 samples of a tile's inputs in LDS
K_CONSUMERS, K_PRODUCERS, K_COVERED = 10, 3, 14 * 4 * 3   # resample_mfma.h
QUAD_MAX_ROUNDS = 2               # resample.hip, kQuadMaxRounds


@pytest.fixture(scope="module")
def sweep():
    t = time.perf_counter()
    plans = capi.resample_plans(P.LO, P.HI)
    took = time.perf_counter() - t
    print(f"\n{len(plans)} plans in {took:.1f} s")
    # designing the coefficients of every rate is ~10^11 evaluations of sin and bessel_i0: hours.  A minute is already
    # far more than the integer arithmetic of the plans needs on any machine.
    assert took < 60, "a plan must cost no coefficient"
    return plans


OLD_RATES = (8000, 11025, 12345, 16000, 22050, 24000, 32000, 44100, 48000, 88200, 96000, 176400, 192000)


def _census(plans):
    """{class: (rates, smallest rate, (smallest L x T, its smallest rate))}, sorted by class."""
    fields = ["family", "mfma_steps", "mf_long_row", "mf_splits", "mf_waves", "vec4", "quad_small", "quad_splits",
              "quad_rounds", "row_mode", "rows_in_lds", "n", "dec_q"]
    cols = np.stack([plans[f] for f in fields], axis=1).astype(np.int64)
    cols[:, 3] = np.minimum(cols[:, 3], 3)                          # workgroups per tile: 1 / 2 / >= 3
    cols[:, 7] = np.minimum(cols[:, 7], 3)
    cols[:, 4] = cols[:, 4] == 10                                   # multiplying waves: 10 / < 10
    uniq, first, inverse, counts = np.unique(cols, axis=0, return_index=True, return_inverse=True, return_counts=True)
    inverse = inverse.reshape(-1)
    cost = plans["L"].astype(np.int64) * plans["T"]
    order = np.lexsort((np.arange(len(cost)), cost, inverse))
    cheapest = order[np.concatenate([[True], inverse[order][1:] != inverse[order][:-1]])]
    out = {}
    for k in range(len(uniq)):
        key = P.class_key(plans[first[k]])
        assert key not in out, key                                  # (the columns and class_key cut alike)
        out[key] = (int(counts[k]), P.LO + int(first[k]), (int(cost[cheapest[k]]), P.LO + int(cheapest[k])))
    return dict(sorted(out.items()))


def test_the_struct_is_the_headers():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "needle_hip.h")).read(), flags=re.S)
    body = text.split("typedef struct NeedleHipResamplePlan {")[1].split("} NeedleHipResamplePlan;")[0]
    names = [n.strip() for decl in re.findall(r"\bint\s+([^;]+);", body) for n in decl.split(",")]
    assert names == capi.RESAMPLE_PLAN_FIELDS
    assert C.sizeof(capi.CResamplePlan) == 4 * len(names) == capi.RESAMPLE_PLAN_DTYPE.itemsize
    enum = text.split("enum NeedleHipResampleFamily {")[1].split("}")[0]
    assert [n.lower() for n in re.findall(r"NEEDLE_HIP_RESAMPLE_(\w+)\s*=", enum)] == capi.RESAMPLE_FAMILIES
    L = capi.lib()
    assert L.needle_hip_resample_plan(48000, None) == capi.ERROR_NAMES.index("NullArgument")
    for bad in (0, -1, 1999, 768001):
        p = capi.CResamplePlan()
        p.L = 7
        assert L.needle_hip_resample_plan(bad, C.byref(p)) == INVALID and p.L == 0 and p.family == 0


def test_ratio_taps_and_output_length_of_every_rate(sweep):
    """L / M is 11025 / rate in lowest terms, T = 2 ceil(16 / min(L / M, 1)) (oracle/ora_resample.c), and a tile is a
    whole number of phase cycles."""
    rates = np.arange(P.LO, P.HI + 1, dtype=np.int64)
    g = np.gcd(rates, P.TARGET)
    L, M = P.TARGET // g, rates // g
    assert (sweep["L"] == L).all() and (sweep["M"] == M).all()
    # in f64 as the oracle computes it, not in integers: at 540225 Hz (L / M = 1 / 49) 16 / (1.0 / 49) is 784.0000000000001
    # and the filter has 785 taps a side, in the oracle and here
    half = np.ceil(16.0 / np.minimum(L.astype(np.float64) / M.astype(np.float64), 1.0)).astype(np.int64)
    half[rates == P.TARGET] = 1
    assert (sweep["T"] == 2 * half).all()
    exact = np.where(M > L, -(-16 * M // L), 16)
    assert (half[rates != P.TARGET] >= exact[rates != P.TARGET]).all() and (half - exact <= 1).all()
    ok = sweep["family"] != FAM["refused"]
    assert (sweep["tile_outputs"][ok] > 0).all() and (sweep["tile_outputs"][ok] % L[ok] == 0).all()
    assert (sweep["tile_outputs"][~ok] == 0).all()
    lib = capi.lib()
    for r in list(range(P.LO, P.HI + 1, 1009)) + P.RATES:
        p = sweep[r - P.LO]
        for n in (0, 1, 12345, 10 ** 7 + 1):
            want = n if r == P.TARGET else -(-n * int(p["L"]) // int(p["M"]))
            assert lib.needle_hip_resample_out_len(n, r) == want


def test_the_tiling_the_feeder_streams_by_is_the_plans(sweep):
    """resample_tiling_host feeds the feeder: an unfinished lane holds the whole tiles whose taps lie inside the samples
    fed (include/needle_hip.h), so the kept items after n samples at `rate` are those of tiles * tile_outputs samples at
    11025 Hz -- one sample before a tile completes and at the sample that completes it.  A refused rate holds nothing."""
    for r in list(range(P.LO, P.HI + 1, 997)) + P.RATES:
        p = sweep[r - P.LO]
        if r == P.TARGET:
            continue
        if p["family"] == FAM["refused"]:
            assert capi.feeder_num_ready(10 ** 7, r) == 0
            continue
        L, M, half, tile = int(p["L"]), int(p["M"]), int(p["T"]) // 2, int(p["tile_outputs"])
        k = max(4, -(-40000 // tile))
        n = half + (k * tile - 1) * M // L + 1                     # smallest n with ceil((n - half) L / M) >= k tile
        assert -(-(n - half) * L // M) >= k * tile > -(-(n - 1 - half) * L // M)
        assert capi.feeder_num_ready(n, r) == capi.feeder_num_ready(k * tile, P.TARGET), r
        assert capi.feeder_num_ready(n - 1, r) == capi.feeder_num_ready((k - 1) * tile, P.TARGET), r
        if tile >= 8192:
            assert capi.feeder_num_ready(n, r) > capi.feeder_num_ready(n - 1, r), r


def test_lds_and_refusal_of_every_rate(sweep):
    """Every launch fits the LDS of a workgroup; a rate is refused exactly when not even one lane per phase fits the
    region (its M inputs, the window, the padding of the shifted rows) or the general kernel's LDS exceeds the limit."""
    fam, M, G = sweep["family"], sweep["M"].astype(np.int64), sweep["groups"].astype(np.int64)
    refused = fam == FAM["refused"]
    assert (sweep["lds_bytes"][~refused] <= LDS_LIMIT).all()
    assert (G >= (sweep["T"] + 3) // 4 + 1).all() and (G % 4 == 0).all()   # a row shifted by up to 3 taps, in fours
    no_lane_fits = M + 4 * G + 8 > MAX_REGION_SAMPLES
    too_much_lds = sweep["lds_bytes"] > LDS_LIMIT
    assert (refused == (no_lane_fits | too_much_lds)).all()
    assert (sweep["lds_bytes"][no_lane_fits] == 0).all() and (sweep["n"][no_lane_fits] == 0).all()
    # the general kernel's LDS, from its layout: samples | the tile's outputs (s16) | eight waves' coefficient rows
    gen = (fam == FAM["general"]) | (fam == FAM["identity"]) | (refused & ~no_lane_fits)
    p = sweep[gen]
    n, Mg, Gg = p["n"].astype(np.int64), p["M"].astype(np.int64), p["groups"].astype(np.int64)
    assert ((n & (n - 1)) == 0).all() and (n >= 1).all()
    row = p["row_mode"] == 1
    assert (row == ((Mg >= 64) & (n <= 32))).all()
    need = np.where(row, n * (Mg + p["T"] + 3), n * Mg + p["T"] + 3)           # samples the tile's lanes read
    assert (4 * p["region_slots"] >= need).all() and (4 * p["region_slots"] <= MAX_REGION_SAMPLES + 8 * n).all()
    assert (p["pitch"][row] % 2 == 1).all() and (p["pitch"][~row] == 0).all()
    assert (p["region_slots"][row] == n[row] * p["pitch"][row]).all()
    assert (4 * p["pitch"][row] >= Mg[row] + 4 * Gg[row]).all()                # a lane's window never leaves its row
    rows_per_wave = np.where(n >= 64, 1, 64 // n)
    scratch = 8 * rows_per_wave * Gg * 16
    # rows through LDS need one shift per phase (row layout, or M % 4 == 0) and a scratch of at most 48 KB
    assert ((p["rows_in_lds"] == 1) == ((row | (Mg % 4 == 0)) & (scratch <= 48 * 1024))).all()
    assert (p["vec4"] == (Mg % 4 == 0)).all()
    tile_bytes = (n * p["L"] * 2 + 15) // 16 * 16
    assert (p["lds_bytes"] == 16 * p["region_slots"] + tile_bytes + np.where(p["rows_in_lds"] == 1, scratch, 0)).all()
    assert (p["tile_outputs"][p["family"] != FAM["refused"]] == (n * p["L"])[p["family"] != FAM["refused"]]).all()


def test_mfma_plans(sweep):
    """resample_mfma.h: a wave owns a block of sixteen outputs; 4 STEPS samples must hold the union of their windows; a
    workgroup has at most kConsumers multiplying waves and every workgroup of a tile has a block; a row longer than the
    kCovered groups its staging threads move is completed from the start of the next row, which needs one workgroup per
    tile, rows at most kCovered groups apart, a duplicated range inside what the next row's threads move, and a tail of
    at most one group per staging thread."""
    idx = np.nonzero(sweep["family"] == FAM["mfma"])[0]
    assert len(idx) > 5000
    for i in idx:
        p = sweep[i]
        L, M, T, S, nb = (int(p[f]) for f in ("L", "M", "T", "mfma_steps", "nblocks"))
        assert M % 4 == 0 and M >= 64 and S in (12, 20, 36, 52) and nb == -(-L // 16)
        o0 = np.arange(nb, dtype=np.int64) * 16
        o1 = np.minimum(o0 + 15, L - 1)
        starts = o0 * M // L                                        # first tap of a block's first output, from the row's
        union = o1 * M // L - starts + T
        assert 4 * S >= union.max(), (P.LO + i, S, union.max())
        assert S == min(b for b in (12, 20, 36, 52) if 4 * b >= union.max()), "a smaller kernel would do"
        splits, waves, groups = int(p["mf_splits"]), int(p["mf_waves"]), int(p["mf_groups"])
        assert 1 <= waves <= K_CONSUMERS and splits * waves >= nb and (splits - 1) * waves < nb
        assert p["blocks_per_tile"] == splits and p["tile_outputs"] == 16 * L and p["threads"] == 1024
        # groups of four samples a workgroup's rows hold: from its first block's window (aligned down) to the end of its last
        delta = (1 - T // 2) % 4
        need = 0
        for sp in range(splits):
            b0, b1 = sp * waves, min((sp + 1) * waves, nb)
            lo = (int(starts[b0]) + delta) // 4 * 4
            need = max(need, -(-(int(starts[b1 - 1]) + delta + 4 * S - lo) // 4))
        assert groups == need
        assert p["lds_bytes"] == 2 * max(groups, K_COVERED) * 4 * 16 * 4          # two buffers of [sample][16 rows] f32
        if groups > K_COVERED:
            assert p["mf_long_row"] == 1 and splits == 1
            lo, hi = int(p["mf_dup_lo"]), int(p["mf_dup_hi"])
            assert lo == K_COVERED - M // 4 >= 0 and hi == groups - M // 4 <= K_COVERED
            assert 0 < hi - lo <= 64 * K_PRODUCERS
        else:
            assert p["mf_long_row"] == 0 and p["mf_dup_lo"] == 0 and p["mf_dup_hi"] == 0


def test_quad_plans(sweep):
    """resample_quad_kernel: sixteen rows of L outputs, a lane computes four consecutive outputs of a row; the quads of a
    row are cut into `splits` workgroups of one DPP row (16 lanes) per quad in whole waves, at most 1024 threads and
    kQuadMaxRounds rounds; the output tile reuses the start of the sample region, so it must fit it."""
    p = sweep[sweep["family"] == FAM["quad"]]
    assert len(p) > 100000
    L, M = p["L"].astype(np.int64), p["M"].astype(np.int64)
    quads = (L + 3) // 4
    qps, threads, splits = p["quads_per_split"].astype(np.int64), p["quad_threads"].astype(np.int64), p["quad_splits"]
    assert (M >= 64).all() and (L >= 4).all()
    assert (splits * qps >= quads).all() and ((splits - 1) * qps < quads).all()          # no empty workgroup
    assert (threads % 64 == 0).all() and (threads <= 1024).all() and (threads == p["threads"]).all()
    assert (qps <= QUAD_MAX_ROUNDS * threads // 16).all()
    assert (p["quad_rounds"] == -(-qps // (threads // 16))).all() and (p["quad_rounds"] <= QUAD_MAX_ROUNDS).all()
    assert (p["quad_small"] == (threads <= 640)).all() and (p["vec4"] == (M % 4 == 0)).all()
    assert (16 * 4 * qps * 2 <= p["lds_bytes"]).all()                                    # the s16 output tile
    assert (p["lds_bytes"] == 16 * p["pitch"] * 16).all() and (p["pitch"] % 2 == 1).all()
    # a row of a workgroup holds the groups from its first quad's first read to its last quad's, the steps, and the two
    # groups of slack the kernel stages: the first workgroup of every rate, every workgroup of every 40th
    first_wg = ((4 * (qps - 1) * M // L + p["delta"]) >> 2) + p["quad_steps"] + 2
    assert (p["pitch"] >= first_wg).all()
    for q in p[::40]:
        Lq, Mq, k, d = int(q["L"]), int(q["M"]), int(q["quads_per_split"]), int(q["delta"])
        nq = (Lq + 3) // 4
        b0 = (np.arange(nq, dtype=np.int64) * 4 * Mq // Lq + d) >> 2
        need = max(int(b0[min(a + k, nq) - 1] - b0[a]) for a in range(0, nq, k)) + int(q["quad_steps"]) + 2
        assert q["pitch"] >= need, (Lq, Mq, need)
    # the steps hold T taps, the 3 M / L samples between a lane's four outputs and the two alignments of up to 3
    assert (4 * p["quad_steps"] >= p["T"] + (3 * M + L - 1) // L + 6).all() and (p["quad_steps"] % 8 == 0).all()
    assert (p["tile_outputs"] == 16 * L).all() and (p["blocks_per_tile"] == splits).all()


def test_census_and_the_gpu_tables_coverage(sweep):
    """Every class of plan the planner selects with the default environment has a rate in the GPU test's table, none
    excepted, and the table's cheapest rate of a class is the cheapest there is (smallest L x T: small tables)."""
    census = _census(sweep)
    print("\nclass | rates | smallest rate | smallest L x T at")
    for key, (count, first, (cost, at)) in census.items():
        print(" ".join(key), "|", count, "|", first, "|", cost, "at", at)
    total, refused = len(sweep), census[("refused",)][0]
    print(f"{len(census) - 1} classes with a kernel; {refused} of {total} rates refused ({100.0 * refused / total:.1f} %)")
    assert sum(c[0] for c in census.values()) == total
    assert len(set(P.RATES)) == len(P.RATES)
    table = {}
    for r in P.RATES:
        table.setdefault(P.class_key(sweep[r - P.LO]), []).append(r)
    assert ("refused",) not in table, table.get(("refused",))
    missing = [key for key in census if key != ("refused",) and key not in table]
    assert not missing, f"no rate of tests/resample_plans.py takes the plan(s) {missing}; their smallest rates: " \
                        f"{[census[k][1] for k in missing]}"
    for key, rates in table.items():
        have = min(int(sweep["L"][r - P.LO]) * int(sweep["T"][r - P.LO]) for r in rates)
        assert have == census[key][2][0], (key, rates, census[key][2])
    before = {P.class_key(sweep[r - P.LO]) for r in OLD_RATES}
    print(f"the thirteen rates of the older tests take {len(before)} classes; the table's {len(P.RATES)} take {len(table)}")


def _boundary(sweep):
    rates = np.arange(P.LO, P.HI + 1)
    coprime = np.gcd(rates, P.TARGET) == 1
    accepted = coprime & (sweep["family"] != FAM["refused"])
    last = int(rates[accepted].max())
    nxt = int(rates[coprime & (rates > last)].min())
    return last, nxt


def test_refusal_boundary_of_rates_coprime_to_11025(sweep):
    last, nxt = _boundary(sweep)
    print(f"\nlargest accepted rate coprime to 11025: {last}; the next coprime rate, {nxt}, is refused")
    assert last in P.RATES, "the GPU test's table lacks the boundary rate"
    rates = np.arange(P.LO, P.HI + 1)
    coprime = np.gcd(rates, P.TARGET) == 1
    assert (sweep["family"][coprime & (rates > last)] == FAM["refused"]).all()
    assert capi.resample_plan(last)["family"] != "refused" and capi.resample_plan(last)["L"] == P.TARGET
    L = capi.lib()
    p = capi.CResamplePlan()
    assert L.needle_hip_resample_plan(nxt, C.byref(p)) == INVALID and p.family == FAM["refused"]
    assert (p.L, p.M) == (P.TARGET, nxt) and p.tile_outputs == 0 and p.lds_bytes == 0
    assert "rate ratio too large" in L.needle_hip_last_error_message().decode()
    with pytest.raises(capi.NeedleError) as e:
        capi.resample_plan(nxt)
    assert e.value.name == "InvalidArgument"
    assert capi.resample_plan(nxt, refused_ok=True)["family"] == "refused"


def test_refused_rates_cost_nothing_and_allocate_nothing(sweep):
    """The refusal comes before any coefficient: a thousand refusals of rates whose L x T is a million or more each take
    less time than designing one of them would, and the process does not grow."""
    import resource
    _, nxt = _boundary(sweep)
    rates = np.arange(P.LO, P.HI + 1)
    big = rates[(sweep["family"] == FAM["refused"]) & (sweep["L"].astype(np.int64) * sweep["T"] >= 10 ** 6)][:1000]
    assert len(big) == 1000
    L = capi.lib()
    p = capi.CResamplePlan()
    L.needle_hip_resample_plan(int(big[0]), C.byref(p))
    rss = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss
    t = time.perf_counter()
    for r in big:
        assert L.needle_hip_resample_plan(int(r), C.byref(p)) == INVALID
        assert capi.feeder_num_ready(10 ** 6, int(r)) == 0
    took = time.perf_counter() - t
    grown = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss - rss
    print(f"\n1000 refusals (plan and feeder tiling) in {took * 1e3:.0f} ms, peak RSS grew {grown} KB")
    assert took < 5.0                                              # (10^9 coefficients would be minutes)
    assert grown < 4096                                            # one such design alone is >= 4 MB of f32


def test_feeder_and_library_refuse_a_refused_rate_at_once(sweep):
    last, nxt = _boundary(sweep)
    f = capi.Feeder.with_formats([(2, last, capi.SAMPLE_S16), (1, 11025, capi.SAMPLE_S16)], 2)
    assert f.lane_format(0) == (2, last, capi.SAMPLE_S16)
    with pytest.raises(capi.NeedleError) as e:
        capi.Feeder.with_formats([(2, 48000, capi.SAMPLE_S16), (1, nxt, capi.SAMPLE_S16)], 2)
    assert e.value.name == "InvalidArgument" and "rate ratio" in str(e.value)
    with pytest.raises(capi.NeedleError) as e:
        capi.Feeder(1, 1, nxt, capi.SAMPLE_S16, 1)
    assert e.value.name == "InvalidArgument"
    lib = capi.Library(3)
    with pytest.raises(capi.NeedleError) as e:
        lib.set_sample_rate(nxt)
    assert e.value.name == "InvalidArgument" and "rate ratio" in str(e.value)
    assert lib.set_sample_rate(last) is lib                         # the refusal left the library usable
    assert capi.lib().needle_hip_library_set_sample_rate(lib._h, 44056) == INVALID


def test_environment_switches_change_the_plan_as_the_launch(monkeypatch):
    for k in ("NEEDLE_HIP_RESAMPLE_V1", "NEEDLE_HIP_RESAMPLE_QUAD", "NEEDLE_HIP_RESAMPLE_SPLITS"):
        monkeypatch.delenv(k, raising=False)
    assert capi.resample_plan(48000)["family"] == "mfma" and capi.resample_plan(12345)["family"] == "quad"
    assert capi.resample_plan(44100)["family"] == "dec"
    monkeypatch.setenv("NEEDLE_HIP_RESAMPLE_QUAD", "1")
    q = capi.resample_plan(48000)
    assert q["family"] == "quad" and q["tile_outputs"] == 16 * 147 and q["vec4"] == 1
    assert capi.resample_plan(12345)["family"] == "quad" and capi.resample_plan(44100)["family"] == "dec"
    monkeypatch.delenv("NEEDLE_HIP_RESAMPLE_QUAD")
    monkeypatch.setenv("NEEDLE_HIP_RESAMPLE_V1", "1")
    for rate in (48000, 12345, 44100):
        g = capi.resample_plan(rate)
        assert g["family"] == "general" and g["tile_outputs"] == g["n"] * g["L"], rate
    g = capi.resample_plan(12345)                                   # row layout, M % 4 != 0: resample_kernel<CH, true, false>
    assert (g["row_mode"], g["rows_in_lds"], g["vec4"]) == (1, 1, 0)
    monkeypatch.delenv("NEEDLE_HIP_RESAMPLE_V1")
    # 12345 Hz: L = 735, 184 quads of a row.  By default twelve workgroups of 16 quads = 256 threads, one round each
    d = capi.resample_plan(12345)
    assert (d["quad_splits"], d["quads_per_split"], d["quad_threads"], d["quad_rounds"], d["quad_small"]) == (12, 16, 256, 1, 1)
    monkeypatch.setenv("NEEDLE_HIP_RESAMPLE_SPLITS", "2")           # 92 quads each: 1024 threads = 64 DPP rows, two rounds
    s = capi.resample_plan(12345)
    assert (s["quad_splits"], s["quads_per_split"], s["quad_threads"], s["quad_rounds"], s["quad_small"]) == (2, 92, 1024, 2, 0)
    assert s["family"] == "quad" and s["blocks_per_tile"] == 2 and s["lds_bytes"] > d["lds_bytes"]
    monkeypatch.setenv("NEEDLE_HIP_RESAMPLE_SPLITS", "1")           # 184 quads need three rounds of 64: not this kernel
    assert capi.resample_plan(12345)["family"] == "general"
    monkeypatch.setenv("NEEDLE_HIP_RESAMPLE_SPLITS", "4")           # 46 quads: 768 threads, the large instantiation, one round
    s = capi.resample_plan(12345)
    assert (s["quads_per_split"], s["quad_threads"], s["quad_rounds"], s["quad_small"]) == (46, 768, 1, 0)


def test_the_signal_of_a_case_meets_its_conditions():
    """tests/resample_plans.py's streams and signal on three cheap plans, against the oracle alone (the GPU test checks
    the same on every case): the output is not constant, the full-scale stretch reaches the clamp, under 1 % of the
    outputs outside it are clamped; a stereo sum is odd about half the time and negative about half the time."""
    from oracle import oracle as O
    for rate in (2205, 9408, 102375):
        p = capi.resample_plan(rate)
        lens = P.stream_lengths(p)
        assert lens[1] == 0 and lens[3] == 1 and lens[5] == p["T"] // 2 - 1
        tile_in = p["tile_outputs"] // p["L"] * p["M"]
        assert lens[0] == 3 * tile_in and lens[2] == tile_in and lens[4] == 3 * tile_in + 1
        out = capi.lib().needle_hip_resample_out_len
        assert out(lens[0], rate) == 3 * p["tile_outputs"] and out(lens[2], rate) == p["tile_outputs"]
        tail = out(lens[6], rate) - 2 * p["tile_outputs"]
        assert 0 < tail < p["tile_outputs"] and tail % 4 != 0 and tail % 16 != 0
        for ch in (1, 2):
            for k, n in enumerate(lens):
                x = P.signal(n, ch, p, 10 * k + ch)
                assert x.dtype == np.int16 and x.size == n * ch
                P.check_reference(O.resample(x, ch, rate), n, p)
                if ch == 2 and n > 1000:
                    a, b = P.stretch_of(n, p)
                    s = np.delete(x[0::2].astype(np.int64) + x[1::2], np.arange(a, b))
                    assert 0.3 < (s % 2 == 1).mean() < 0.7 and 0.3 < (s < 0).mean() < 0.7
                    assert ((s % 2 == 1) & (s < 0)).mean() > 0.1     # where C truncation and floor differ
