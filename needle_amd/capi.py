"""ctypes binding of libneedle_capi.so (include/needle.h + include/needle_hip.h).

The classes mirror needle::audio::{Analyzer, Comparator, FrameHashes} (needle/src/audio/*.rs) over the
C ABI, so tests read like the reference's own usage: build with paths, chain with_* setters, run.
All compute happens in the shared library on the GPU; this module holds no arithmetic and no CPU
fallback — if the library or a HIP device is missing the calls raise.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np

NS = 1_000_000_000
# NEEDLE_CAPI_LIB: another build of the same library (A/B timing of kernel variants)
LIB_PATH = os.environ.get("NEEDLE_CAPI_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "libneedle_capi.so")

ERROR_NAMES = ["Ok", "InvalidUtf8String", "NullArgument", "InvalidArgument", "FrameHashDataNotFound",
               "FrameHashDataInvalidVersion", "InvalidFrameHashData", "ComparatorMinimumPaths",
               "AnalyzerInvalidHashPeriod", "AnalyzerInvalidHashDuration", "IOError", "Unknown"]

# audio/mod.rs:14-45
DEFAULT_HASH_MATCH_THRESHOLD = 10
DEFAULT_OPENING_SEARCH_PERCENTAGE = 0.50
DEFAULT_ENDING_SEARCH_PERCENTAGE = 0.25
DEFAULT_MIN_OPENING_DURATION = 20
DEFAULT_MIN_ENDING_DURATION = 20
DEFAULT_HASH_DURATION = 0.3
MAX_CHANNELS = 8  # NEEDLE_HIP_MAX_CHANNELS: interleaved channels the analyze paths accept


class NeedleError(RuntimeError):
    def __init__(self, code: int, detail: str = ""):
        self.code = code
        self.name = ERROR_NAMES[code] if 0 <= code < len(ERROR_NAMES) else str(code)
        super().__init__(f"NeedleError_{self.name}: {detail}")


class Seq(C.Structure):
    _fields_ = [("offset", C.c_uint32), ("len", C.c_uint32)]


class Problem(C.Structure):
    _fields_ = [("src_seq", C.c_uint32), ("dst_seq", C.c_uint32), ("min_len", C.c_uint32), ("tag", C.c_uint32)]


class Run(C.Structure):
    _fields_ = [("problem", C.c_uint32), ("src_end", C.c_uint32), ("dst_end", C.c_uint32), ("len", C.c_uint32),
                ("src_match_hash", C.c_uint32), ("dst_match_hash", C.c_uint32)]


class CSearchResult(C.Structure):
    _fields_ = [("has_result", C.c_bool), ("has_opening", C.c_bool), ("has_ending", C.c_bool),
                ("opening_start_ns", C.c_uint64), ("opening_end_ns", C.c_uint64),
                ("ending_start_ns", C.c_uint64), ("ending_end_ns", C.c_uint64)]


class CMatchEvidence(C.Structure):                     # NeedleHipMatchEvidence
    _fields_ = [("partner", C.c_uint32), ("is_source", C.c_uint32), ("candidate", C.c_uint32), ("candidates", C.c_uint32),
                ("support", C.c_uint32), ("partners", C.c_uint32), ("score", C.c_float),
                ("match_hash", C.c_uint32), ("partner_hash", C.c_uint32), ("reserved", C.c_uint32),
                ("start_ns", C.c_uint64), ("end_ns", C.c_uint64),
                ("partner_start_ns", C.c_uint64), ("partner_end_ns", C.c_uint64)]


class CSearchEvidence(C.Structure):                    # NeedleHipSearchEvidence
    _fields_ = [("opening", CMatchEvidence), ("ending", CMatchEvidence)]


NO_PARTNER = 0xFFFFFFFF                                # NeedleHipMatchEvidence.partner of a region without a match


RUN_DTYPE = np.dtype([("problem", "<u4"), ("src_end", "<u4"), ("dst_end", "<u4"), ("len", "<u4"),
                      ("src_match_hash", "<u4"), ("dst_match_hash", "<u4")])
RUN_WORDS = 6

# Every symbol include/needle.h and include/needle_hip.h declare (tests check the library exports all).
NEEDLE_H_SYMBOLS = [
    "needle_error_to_str", "needle_util_find_video_files", "needle_util_video_files_free",
    "needle_audio_analyzer_new_default", "needle_audio_analyzer_new", "needle_audio_analyzer_get_frame_hashes",
    "needle_audio_analyzer_free", "needle_audio_analyzer_print_paths", "needle_audio_analyzer_run",
    "needle_audio_comparator_new_default", "needle_audio_comparator_new", "needle_audio_comparator_free",
    "needle_audio_comparator_run"]
NEEDLE_HIP_H_SYMBOLS = [
    "needle_hip_device_count", "needle_hip_set_device", "needle_hip_synchronize", "needle_hip_stream",
    "needle_hip_device_pci_bus_id", "needle_hip_fingerprint_cert_stats", "needle_hip_scan_issued_evaluations",
    "needle_hip_last_error_message",
    "needle_hip_version", "needle_hip_malloc", "needle_hip_free", "needle_hip_memcpy_h2d", "needle_hip_memcpy_d2h",
    "needle_hip_host_free", "needle_hip_last_kernel_ms", "needle_hip_set_kernel_timing", "needle_hip_kernel_launches", "needle_hip_fingerprint_sample_rate",
    "needle_hip_fingerprint_delay_ms", "needle_hip_fingerprint_item_duration_ms", "needle_hip_fingerprint_num_items",
    "needle_hip_fingerprint_num_kept", "needle_hip_fingerprint_host", "needle_hip_fingerprint_device",
    "needle_hip_fingerprint_debug", "needle_hip_fingerprint_stages_debug", "needle_hip_resample_out_len", "needle_hip_resample_host", "needle_hip_resample_plan",
    "needle_hip_downmix_host",
    "needle_hip_hamming_runs_device", "needle_hip_hamming_runs_host",
    "needle_hip_frame_hashes_new", "needle_hip_frame_hashes_free", "needle_hip_frame_hashes_len",
    "needle_hip_frame_hashes_copy", "needle_hip_frame_hashes_hash_duration_ns", "needle_hip_frame_hashes_md5",
    "needle_hip_frame_hashes_read", "needle_hip_frame_hashes_write", "needle_hip_header_md5",
    "needle_hip_analyzer_run_pcm", "needle_hip_comparator_run_with_frame_hashes", "needle_hip_library_new",
    "needle_hip_library_free", "needle_hip_library_include_endings", "needle_hip_library_set_sample_rate",
    "needle_hip_library_rows_per_video",
    "needle_hip_library_set_pcm", "needle_hip_library_set_pcm_device", "needle_hip_library_rank_videos",
    "needle_hip_library_analyze",
    "needle_hip_library_hash_arena", "needle_hip_library_use_hash_arena", "needle_hip_library_num_pairs", "needle_hip_library_search",
    "needle_hip_library_fetch_runs_begin", "needle_hip_library_fetch_runs_end",
    "needle_hip_library_finalize", "needle_hip_library_frame_hashes",
    "needle_hip_comm_create_id", "needle_hip_comm_init", "needle_hip_comm_finalize", "needle_hip_comm_rank",
    "needle_hip_comm_world_size", "needle_hip_comm_backend", "needle_hip_comm_barrier",
    "needle_hip_comm_all_gather_host", "needle_hip_comm_shard", "needle_hip_library_job_begin",
    "needle_hip_library_job_end", "needle_hip_library_stream_pcm", "needle_hip_host_alloc",
    "needle_hip_host_alloc_free", "needle_hip_int_valu_ceiling",
    "needle_hip_comparator_results_from_runs", "needle_hip_library_job_runs", "needle_hip_library_job_comm_bytes",
    "needle_hip_library_job_form",
    "needle_hip_host_threads", "needle_hip_fingerprint_audit_device", "needle_hip_library_audit",
    "needle_hip_scan_counts", "needle_hip_scan_last_launch", "needle_hip_epilogue_host_fallbacks",
    "needle_hip_index_new", "needle_hip_index_free", "needle_hip_index_len", "needle_hip_index_add",
    "needle_hip_index_results", "needle_hip_index_pairs_searched", "needle_hip_index_remove", "needle_hip_index_replace",
    "needle_hip_index_store_sizes", "needle_hip_index_crossmatcher_new", "needle_hip_index_add_matched",
    "needle_hip_index_pairs_scanned", "needle_hip_comparator_results_from_runs_evidence", "needle_hip_index_evidence",
    "needle_hip_group_pairs", "needle_hip_comparator_run_with_frame_hashes_grouped",
    "needle_hip_comparator_results_from_runs_grouped", "needle_hip_comparator_run_grouped",
    "needle_hip_convert_host", "needle_hip_analyzer_run_pcm_format", "needle_hip_library_set_sample_format",
    "needle_hip_feeder_new", "needle_hip_feeder_free", "needle_hip_feeder_feed", "needle_hip_feeder_finish",
    "needle_hip_feeder_reset", "needle_hip_feeder_ready", "needle_hip_feeder_items", "needle_hip_feeder_frame_hashes",
    "needle_hip_feeder_state_bytes", "needle_hip_feeder_num_ready", "needle_hip_feeder_set_audit", "needle_hip_feeder_audit",
    "needle_hip_library_set_video_formats", "needle_hip_library_video_format", "needle_hip_analyzer_run_pcm_formats",
    "needle_hip_feeder_new_lanes", "needle_hip_feeder_lane_format", "needle_hip_feeder_reset_format", "needle_hip_convert_mono_host",
    "needle_hip_channel_mix_default", "needle_hip_rematrix_host", "needle_hip_analyzer_set_channel_mix",
    "needle_hip_analyzer_set_layout_downmix", "needle_hip_comparator_set_layout_downmix", "needle_hip_library_set_channel_mix",
    "needle_hip_feeder_set_lane_mix",
    "needle_hip_feeder_switch_format", "needle_hip_feeder_lane_segments", "needle_hip_feeder_num_ready_segments",
    "needle_hip_matcher_new", "needle_hip_matcher_free", "needle_hip_matcher_feed", "needle_hip_matcher_feed_from_feeder",
    "needle_hip_matcher_finish", "needle_hip_matcher_reset", "needle_hip_matcher_ready", "needle_hip_matcher_runs",
    "needle_hip_matcher_open", "needle_hip_matcher_stats", "needle_hip_matcher_new_regions",
    "needle_hip_index_matcher_new", "needle_hip_index_add_streamed",
    "needle_hip_index_new_grouped", "needle_hip_index_add_grouped", "needle_hip_index_groups",
    "needle_hip_crossmatcher_new", "needle_hip_crossmatcher_free", "needle_hip_crossmatcher_feed",
    "needle_hip_crossmatcher_feed_from_feeder", "needle_hip_crossmatcher_finish", "needle_hip_crossmatcher_ready",
    "needle_hip_crossmatcher_lane", "needle_hip_crossmatcher_runs", "needle_hip_crossmatcher_stats",
    "needle_hip_crossmatcher_state_bytes", "needle_hip_crossmatcher_new_regions",
    "needle_hip_crossmatcher_state_bytes_regions", "needle_hip_crossmatcher_shape",
    "needle_hip_crossmatcher_new_resident", "needle_hip_crossmatcher_state_bytes_resident", "needle_hip_crossmatcher_resident",
    "needle_hip_crossmatcher_new_grouped", "needle_hip_crossmatcher_state_bytes_grouped", "needle_hip_crossmatcher_groups",
    "needle_hip_index_crossmatcher_new_grouped", "needle_hip_index_add_matched_grouped",
    "needle_hip_library_set_groups", "needle_hip_library_groups",
    "needle_hip_fingerprint_compressed_bound", "needle_hip_fingerprint_compress_host", "needle_hip_fingerprint_decompress_host",
    "needle_hip_feeder_compressed", "needle_hip_fingerprint_base64_encode", "needle_hip_fingerprint_base64_decode",
    "needle_hip_fingerprint_codec_tiles", "needle_hip_fingerprint_simhash"]

# enum NeedleHipSampleFormat (FFmpeg's AVSampleFormat numbering): interleaved 0-4, planar (one plane per channel) 5-9
SAMPLE_U8, SAMPLE_S16, SAMPLE_S32, SAMPLE_F32, SAMPLE_F64 = 0, 1, 2, 3, 4
SAMPLE_U8P, SAMPLE_S16P, SAMPLE_S32P, SAMPLE_F32P, SAMPLE_F64P = 5, 6, 7, 8, 9
_SAMPLE_DTYPES = [np.uint8, np.int16, np.int32, np.float32, np.float64]


def sample_format_dtype(sample_format: int):
    """numpy dtype of one sample of `sample_format`."""
    if not 0 <= sample_format <= 9:
        raise ValueError(f"unknown sample format {sample_format}")
    return np.dtype(_SAMPLE_DTYPES[sample_format % 5])


def sample_format_planar(sample_format: int) -> bool:
    return sample_format >= SAMPLE_U8P


def _format_pointers(pcm, channels: int, sample_format: int):
    """(arrays to keep alive, flat pointer list) of streams in `sample_format`: an interleaved stream is one array, a
    planar one a sequence of `channels` planes (or a 2-D array [channels][frames]); None stays NULL (all planes)."""
    dtype = sample_format_dtype(sample_format)
    keep, ptrs = [], []
    for p in pcm:
        if not sample_format_planar(sample_format):
            a = None if p is None else np.ascontiguousarray(p, dtype=dtype)
            keep.append(a)
            ptrs.append(None if a is None else a.ctypes.data)
        elif p is None:
            ptrs += [None] * channels
        else:
            planes = [np.ascontiguousarray(q, dtype=dtype) for q in p]
            if len(planes) != channels:
                raise ValueError(f"a planar stream needs {channels} planes, got {len(planes)}")
            keep += planes
            ptrs += [q.ctypes.data for q in planes]
    return keep, ptrs


class CLaneFormat(C.Structure):                          # NeedleHipLaneFormat
    _fields_ = [("channels", C.c_int32), ("sample_rate", C.c_int32), ("format", C.c_int32)]


class CSegment(C.Structure):                             # NeedleHipSegment
    _fields_ = [("format", CLaneFormat), ("frames", C.c_uint64)]


class ChannelMix(C.Structure):                           # NeedleHipChannelMix
    """A 2 x C matrix of Q15 integers, coef[0][c] to the left output and coef[1][c] to the right (needle_hip.h "Channel
    mixes").  ChannelMix.of(left, right) builds one from two rows; channels == 0 (ChannelMix()) means "no mix"."""
    _fields_ = [("channels", C.c_int32), ("coef", (C.c_int32 * MAX_CHANNELS) * 2)]

    @classmethod
    def of(cls, left: Sequence[int], right: Sequence[int], channels: Optional[int] = None) -> "ChannelMix":
        if len(left) != len(right) or len(left) > MAX_CHANNELS:
            raise ValueError(f"two rows of at most {MAX_CHANNELS} coefficients each")
        m = cls()
        m.channels = len(left) if channels is None else channels
        for c, (l, r) in enumerate(zip(left, right)):
            m.coef[0][c], m.coef[1][c] = int(l), int(r)
        return m

    def rows(self) -> Tuple[List[int], List[int]]:
        n = max(0, min(self.channels, MAX_CHANNELS))
        return list(self.coef[0][:n]), list(self.coef[1][:n])


def channel_mix_default(channel_mask: int) -> ChannelMix:
    """needle_hip_channel_mix_default: the default mix of a WAVEFORMATEXTENSIBLE / FFmpeg channel mask (host arithmetic)."""
    m = ChannelMix()
    check(lib().needle_hip_channel_mix_default(channel_mask, C.byref(m)))
    return m


def _channel_mixes(mixes):
    """NeedleHipChannelMix array; None stands for "no mix" (channels == 0)."""
    arr = (ChannelMix * max(len(mixes), 1))()
    for i, m in enumerate(mixes):
        if m is not None:
            C.memmove(C.byref(arr[i]), C.byref(m), C.sizeof(ChannelMix))
    return arr


RESAMPLE_FAMILIES = ["identity", "dec", "mfma", "quad", "general", "refused"]   # enum NeedleHipResampleFamily
RESAMPLE_PLAN_FIELDS = [
    "family", "L", "M", "T", "tile_outputs", "blocks_per_tile", "threads", "lds_bytes", "n", "row_mode", "rows_in_lds",
    "vec4", "groups", "pitch", "region_slots", "delta", "mfma_steps", "nblocks", "mf_splits", "mf_waves", "mf_groups",
    "mf_long_row", "mf_dup_lo", "mf_dup_hi", "quad_splits", "quads_per_split", "quad_threads", "quad_rounds",
    "quad_small", "quad_steps", "dec_q"]


class CResamplePlan(C.Structure):                        # NeedleHipResamplePlan: plain ints
    _fields_ = [(f, C.c_int) for f in RESAMPLE_PLAN_FIELDS]


RESAMPLE_PLAN_DTYPE = np.dtype([(f, "<i4") for f in RESAMPLE_PLAN_FIELDS])


def _lane_formats(formats):
    """NeedleHipLaneFormat array of (channels, sample_rate, sample_format) triples."""
    return (CLaneFormat * max(len(formats), 1))(*[CLaneFormat(int(c), int(r), int(f)) for c, r, f in formats])


def _lane_pointers(pcm, formats):
    """(arrays to keep alive, flat pointer list, values per stream) of streams that each have a format of their own: the
    concatenation, stream after stream, of each stream's planes -- 1 pointer for an interleaved stream, `channels` for a
    planar one."""
    keep, flat, sizes = [], [], []
    for p, (channels, _, sample_format) in zip(pcm, formats):
        k, f = _format_pointers([p], channels, sample_format)
        keep += k
        flat += f
        sizes.append(0 if p is None else (sum(np.size(q) for q in p) if sample_format_planar(sample_format) else np.size(p)))
    return keep, flat, sizes

_LIB = None


def lib():
    """Loads libneedle_capi.so; raises if it has not been built (no fallback)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'`")
    L = C.CDLL(LIB_PATH)
    vp, sz, u32, u64, b, f32 = C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint64, C.c_bool, C.c_float
    pp = C.POINTER(C.c_char_p)
    L.needle_error_to_str.argtypes = [C.c_int]
    L.needle_error_to_str.restype = C.c_char_p
    L.needle_util_find_video_files.argtypes = [pp, sz, b, b, C.POINTER(pp), C.POINTER(sz)]
    L.needle_util_video_files_free.argtypes = [pp, sz]
    L.needle_util_video_files_free.restype = None
    L.needle_audio_analyzer_new_default.argtypes = [pp, sz, C.POINTER(vp)]
    L.needle_audio_analyzer_new.argtypes = [pp, sz, f32, f32, b, b, b, C.POINTER(vp)]
    L.needle_audio_analyzer_get_frame_hashes.argtypes = [vp, sz, C.POINTER(vp)]
    L.needle_audio_analyzer_free.argtypes = [vp]
    L.needle_audio_analyzer_free.restype = None
    L.needle_audio_analyzer_print_paths.argtypes = [vp]
    L.needle_audio_analyzer_print_paths.restype = None
    L.needle_audio_analyzer_run.argtypes = [vp, f32, b, b]
    L.needle_audio_comparator_new_default.argtypes = [pp, sz, C.POINTER(vp)]
    L.needle_audio_comparator_new.argtypes = [pp, sz, b, C.c_uint16, C.c_uint16, C.c_uint16, f32, C.POINTER(vp)]
    L.needle_audio_comparator_free.argtypes = [vp]
    L.needle_audio_comparator_free.restype = None
    L.needle_audio_comparator_run.argtypes = [vp, b, b, b, b, b]

    L.needle_hip_device_count.argtypes = [C.POINTER(C.c_int)]
    L.needle_hip_set_device.argtypes = [C.c_int]
    L.needle_hip_last_error_message.restype = C.c_char_p
    L.needle_hip_version.restype = C.c_char_p
    L.needle_hip_malloc.argtypes = [C.POINTER(vp), sz]
    L.needle_hip_free.argtypes = [vp]
    L.needle_hip_memcpy_h2d.argtypes = [vp, vp, sz]
    L.needle_hip_memcpy_d2h.argtypes = [vp, vp, sz]
    L.needle_hip_host_free.argtypes = [vp]
    L.needle_hip_host_free.restype = None
    L.needle_hip_last_kernel_ms.argtypes = [C.c_char_p]
    L.needle_hip_last_kernel_ms.restype = C.c_double
    L.needle_hip_kernel_launches.argtypes = [C.c_char_p]
    L.needle_hip_kernel_launches.restype = sz
    L.needle_hip_set_kernel_timing.argtypes = [C.c_char_p]
    L.needle_hip_set_kernel_timing.restype = None
    L.needle_hip_fingerprint_sample_rate.restype = C.c_int
    L.needle_hip_fingerprint_delay_ms.restype = C.c_int
    L.needle_hip_fingerprint_item_duration_ms.restype = C.c_int
    L.needle_hip_fingerprint_num_items.argtypes = [sz]
    L.needle_hip_fingerprint_num_items.restype = sz
    L.needle_hip_fingerprint_num_kept.argtypes = [sz, u32]
    L.needle_hip_fingerprint_num_kept.restype = sz
    L.needle_hip_fingerprint_host.argtypes = [C.POINTER(vp), C.POINTER(sz), sz, C.c_int, u32, C.POINTER(vp)]
    L.needle_hip_fingerprint_device.argtypes = [vp, C.POINTER(u64), C.POINTER(u64), sz, C.c_int, u32, vp,
                                                C.POINTER(u64), b]
    L.needle_hip_fingerprint_debug.argtypes = [vp, sz, C.c_int, vp, vp]
    L.needle_hip_resample_out_len.argtypes = [sz, C.c_int]
    L.needle_hip_resample_out_len.restype = sz
    L.needle_hip_resample_plan.argtypes = [C.c_int, C.POINTER(CResamplePlan)]
    L.needle_hip_resample_host.argtypes = [C.POINTER(vp), C.POINTER(sz), sz, C.c_int, C.c_int, C.POINTER(vp)]
    L.needle_hip_downmix_host.argtypes = [C.POINTER(vp), C.POINTER(sz), sz, C.c_int, C.POINTER(vp)]
    L.needle_hip_convert_host.argtypes = [C.POINTER(vp), C.POINTER(sz), sz, C.c_int, C.c_int, C.POINTER(vp)]
    L.needle_hip_hamming_runs_device.argtypes = [vp, C.POINTER(Seq), sz, C.POINTER(Problem), sz, u32, vp, u32, vp, b]
    L.needle_hip_hamming_runs_host.argtypes = [vp, sz, C.POINTER(Seq), sz, C.POINTER(Problem), sz, u32,
                                               C.POINTER(C.POINTER(Run)), C.POINTER(sz)]
    L.needle_hip_frame_hashes_new.argtypes = [vp, vp, sz, vp, vp, sz, u64, C.c_char_p, C.POINTER(vp)]
    L.needle_hip_frame_hashes_free.argtypes = [vp]
    L.needle_hip_frame_hashes_free.restype = None
    L.needle_hip_frame_hashes_len.argtypes = [vp, b]
    L.needle_hip_frame_hashes_len.restype = sz
    L.needle_hip_frame_hashes_copy.argtypes = [vp, b, vp, vp, sz]
    L.needle_hip_frame_hashes_hash_duration_ns.argtypes = [vp]
    L.needle_hip_frame_hashes_hash_duration_ns.restype = u64
    L.needle_hip_frame_hashes_md5.argtypes = [vp]
    L.needle_hip_frame_hashes_md5.restype = C.c_char_p
    L.needle_hip_frame_hashes_read.argtypes = [C.c_char_p, C.POINTER(vp)]
    L.needle_hip_frame_hashes_write.argtypes = [vp, C.c_char_p]
    L.needle_hip_header_md5.argtypes = [C.c_char_p, C.c_char_p]
    L.needle_hip_analyzer_run_pcm.argtypes = [vp, C.POINTER(vp), C.POINTER(sz), C.c_int, C.c_int, f32, b]
    L.needle_hip_analyzer_run_pcm_format.argtypes = [vp, C.POINTER(vp), C.POINTER(sz), C.c_int, C.c_int, C.c_int, f32, b]
    L.needle_hip_comparator_run_with_frame_hashes.argtypes = [vp, C.POINTER(vp), sz, b, b, b,
                                                              C.POINTER(CSearchResult)]
    L.needle_hip_group_pairs.argtypes = [vp, sz, vp, sz, C.POINTER(C.c_uint64)]
    L.needle_hip_comparator_run_with_frame_hashes_grouped.argtypes = [vp, C.POINTER(vp), sz, vp, b, b, b, C.POINTER(CSearchResult)]
    L.needle_hip_comparator_results_from_runs_grouped.argtypes = [vp, C.POINTER(vp), sz, vp, vp, sz, C.POINTER(CSearchResult)]
    L.needle_hip_comparator_run_grouped.argtypes = [vp, vp, sz, b, b, b, b]
    L.needle_hip_comparator_results_from_runs.argtypes = [vp, C.POINTER(vp), sz, vp, sz, sz, sz,
                                                          C.POINTER(CSearchResult)]
    L.needle_hip_comparator_results_from_runs_evidence.argtypes = [vp, C.POINTER(vp), sz, vp, sz, sz, sz,
                                                                   C.POINTER(CSearchResult), C.POINTER(CSearchEvidence)]
    L.needle_hip_library_new.argtypes = [sz, f32, f32, C.POINTER(vp)]
    L.needle_hip_library_free.argtypes = [vp]
    L.needle_hip_library_free.restype = None
    L.needle_hip_library_include_endings.argtypes = [vp, f32]
    L.needle_hip_library_set_sample_rate.argtypes = [vp, C.c_int]
    L.needle_hip_library_set_sample_format.argtypes = [vp, C.c_int]
    L.needle_hip_library_set_groups.argtypes = [vp, C.POINTER(u32), sz]
    L.needle_hip_library_groups.argtypes = [vp, C.POINTER(u32), sz]
    L.needle_hip_library_rows_per_video.argtypes = [vp]
    L.needle_hip_library_rows_per_video.restype = sz
    L.needle_hip_library_set_pcm.argtypes = [vp, C.POINTER(vp), C.POINTER(sz), C.c_int]
    L.needle_hip_library_analyze.argtypes = [vp, sz, sz, b]
    L.needle_hip_library_hash_arena.argtypes = [vp, C.POINTER(vp), C.POINTER(sz)]
    L.needle_hip_library_use_hash_arena.argtypes = [vp, vp, sz, sz]
    L.needle_hip_library_num_pairs.argtypes = [vp]
    L.needle_hip_library_num_pairs.restype = sz
    L.needle_hip_library_search.argtypes = [vp, vp, sz, sz, vp, u32, vp, b]
    L.needle_hip_library_fetch_runs_begin.argtypes = [vp, C.c_int, vp, vp, u32]
    L.needle_hip_library_fetch_runs_end.argtypes = [vp, C.c_int, C.POINTER(vp), C.POINTER(u32)]
    L.needle_hip_library_finalize.argtypes = [vp, vp, vp, sz, C.POINTER(CSearchResult)]
    L.needle_hip_library_frame_hashes.argtypes = [vp, sz, C.POINTER(vp)]
    L.needle_hip_comm_create_id.argtypes = [vp]
    L.needle_hip_comm_init.argtypes = [vp, C.c_int, C.c_int]
    L.needle_hip_comm_finalize.restype = None
    L.needle_hip_comm_backend.restype = C.c_char_p
    L.needle_hip_comm_all_gather_host.argtypes = [vp, vp, sz]
    L.needle_hip_comm_shard.argtypes = [sz, C.c_int, C.c_int, C.POINTER(sz), C.POINTER(sz)]
    L.needle_hip_comm_shard.restype = None
    L.needle_hip_library_stream_pcm.argtypes = [vp, C.POINTER(vp), C.POINTER(sz), C.c_int]
    L.needle_hip_host_alloc.argtypes = [C.POINTER(vp), sz]
    L.needle_hip_host_alloc_free.argtypes = [vp]
    L.needle_hip_library_job_begin.argtypes = [vp, vp, C.c_int]
    L.needle_hip_library_job_end.argtypes = [vp, vp, C.c_int, C.POINTER(CSearchResult), C.POINTER(sz)]
    L.needle_hip_index_new.argtypes = [vp, C.POINTER(vp)]
    L.needle_hip_index_free.argtypes = [vp]
    L.needle_hip_index_free.restype = None
    L.needle_hip_index_len.argtypes = [vp]
    L.needle_hip_index_len.restype = sz
    L.needle_hip_index_add.argtypes = [vp, C.POINTER(vp), sz]
    L.needle_hip_index_results.argtypes = [vp, C.POINTER(CSearchResult), sz]
    L.needle_hip_index_evidence.argtypes = [vp, C.POINTER(CSearchEvidence), sz]
    L.needle_hip_index_pairs_searched.argtypes = [vp, C.POINTER(u64), C.POINTER(u64)]
    L.needle_hip_index_pairs_scanned.argtypes = [vp, C.POINTER(u64), C.POINTER(u64)]
    L.needle_hip_index_crossmatcher_new.argtypes = [vp, sz, C.POINTER(sz), C.POINTER(u32), C.POINTER(vp)]
    L.needle_hip_index_add_matched.argtypes = [vp, vp, C.POINTER(vp), sz]
    L.needle_hip_index_crossmatcher_new_grouped.argtypes = [vp, sz, C.POINTER(u32), C.POINTER(sz), C.POINTER(u32), C.POINTER(vp)]
    L.needle_hip_index_add_matched_grouped.argtypes = [vp, vp, C.POINTER(vp), sz]
    L.needle_hip_index_matcher_new.argtypes = [vp, sz, C.POINTER(vp)]
    L.needle_hip_index_add_streamed.argtypes = [vp, vp, vp, C.POINTER(vp), sz]
    L.needle_hip_index_new_grouped.argtypes = [vp, C.POINTER(vp)]
    L.needle_hip_index_add_grouped.argtypes = [vp, C.POINTER(vp), C.POINTER(u32), sz]
    L.needle_hip_index_groups.argtypes = [vp, C.POINTER(u32), sz]
    L.needle_hip_feeder_new.argtypes = [sz, C.c_int, C.c_int, C.c_int, u32, C.POINTER(vp)]
    L.needle_hip_feeder_free.argtypes = [vp]
    L.needle_hip_feeder_free.restype = None
    L.needle_hip_feeder_feed.argtypes = [vp, C.POINTER(vp), C.POINTER(sz)]
    L.needle_hip_feeder_finish.argtypes = [vp, C.POINTER(sz), sz]
    L.needle_hip_feeder_reset.argtypes = [vp, C.POINTER(sz), sz]
    L.needle_hip_feeder_ready.argtypes = [vp, sz, C.POINTER(sz), C.POINTER(u64), C.POINTER(b)]
    L.needle_hip_feeder_items.argtypes = [vp, sz, sz, sz, vp]
    L.needle_hip_feeder_frame_hashes.argtypes = [vp, sz, sz, u64, f32, C.c_char_p, C.POINTER(vp)]
    L.needle_hip_feeder_state_bytes.argtypes = [vp, C.POINTER(u64)]
    L.needle_hip_feeder_set_audit.argtypes = [vp, b]
    L.needle_hip_feeder_audit.argtypes = [vp, sz, vp]
    L.needle_hip_feeder_num_ready.argtypes = [u64, C.c_int, C.c_int, u32, b]
    L.needle_hip_feeder_num_ready.restype = sz
    L.needle_hip_feeder_new_lanes.argtypes = [vp, sz, u32, C.POINTER(vp)]
    L.needle_hip_fingerprint_compressed_bound.argtypes = [sz]
    L.needle_hip_fingerprint_compressed_bound.restype = sz
    L.needle_hip_fingerprint_compress_host.argtypes = [vp, C.POINTER(u64), sz, C.c_int, C.POINTER(vp), C.POINTER(u64)]
    L.needle_hip_fingerprint_decompress_host.argtypes = [vp, C.POINTER(u64), sz, C.POINTER(vp), C.POINTER(u64), vp, vp]
    L.needle_hip_feeder_compressed.argtypes = [vp, sz, C.c_int, C.POINTER(vp), C.POINTER(sz)]
    L.needle_hip_fingerprint_base64_encode.argtypes = [vp, sz, C.POINTER(vp), C.POINTER(sz)]
    L.needle_hip_fingerprint_base64_decode.argtypes = [vp, sz, C.POINTER(vp), C.POINTER(sz)]
    L.needle_hip_fingerprint_codec_tiles.argtypes = [C.POINTER(sz), C.POINTER(sz)]
    L.needle_hip_fingerprint_simhash.argtypes = [vp, sz, C.POINTER(u32)]
    L.needle_hip_feeder_lane_format.argtypes = [vp, sz, vp]
    L.needle_hip_library_set_video_formats.argtypes = [vp, vp, vp]
    L.needle_hip_library_video_format.argtypes = [vp, sz, vp]
    L.needle_hip_analyzer_run_pcm_formats.argtypes = [vp, C.POINTER(vp), C.POINTER(sz), vp, vp, f32, b]
    L.needle_hip_feeder_reset_format.argtypes = [vp, C.POINTER(sz), vp, sz]
    L.needle_hip_convert_mono_host.argtypes = [C.POINTER(vp), C.POINTER(sz), vp, sz, C.POINTER(vp)]
    L.needle_hip_channel_mix_default.argtypes = [u32, vp]
    L.needle_hip_rematrix_host.argtypes = [C.POINTER(vp), C.POINTER(sz), vp, vp, sz, C.POINTER(vp)]
    L.needle_hip_analyzer_set_channel_mix.argtypes = [vp, vp]
    L.needle_hip_analyzer_set_layout_downmix.argtypes = [vp, b]
    L.needle_hip_comparator_set_layout_downmix.argtypes = [vp, b]
    L.needle_hip_library_set_channel_mix.argtypes = [vp, vp]
    L.needle_hip_feeder_set_lane_mix.argtypes = [vp, C.POINTER(sz), vp, sz]
    L.needle_hip_feeder_switch_format.argtypes = [vp, C.POINTER(sz), vp, vp, sz]
    L.needle_hip_feeder_lane_segments.argtypes = [vp, sz, vp, sz, C.POINTER(sz)]
    L.needle_hip_feeder_num_ready_segments.argtypes = [vp, sz, u32, b]
    L.needle_hip_feeder_num_ready_segments.restype = sz
    L.needle_hip_matcher_new.argtypes = [vp, sz, vp, vp, sz, sz, u32, C.POINTER(vp)]
    L.needle_hip_matcher_new_regions.argtypes = [vp, sz, vp, vp, sz, sz, sz, u32, C.POINTER(vp)]
    L.needle_hip_matcher_free.argtypes = [vp]
    L.needle_hip_matcher_free.restype = None
    L.needle_hip_matcher_feed.argtypes = [vp, C.POINTER(vp), C.POINTER(sz)]
    L.needle_hip_matcher_feed_from_feeder.argtypes = [vp, vp]
    L.needle_hip_matcher_finish.argtypes = [vp, C.POINTER(sz), sz]
    L.needle_hip_matcher_reset.argtypes = [vp, C.POINTER(sz), sz]
    L.needle_hip_matcher_ready.argtypes = [vp, sz, C.POINTER(sz), C.POINTER(u64), C.POINTER(b)]
    L.needle_hip_matcher_runs.argtypes = [vp, sz, sz, sz, vp]
    L.needle_hip_matcher_open.argtypes = [vp, sz, C.POINTER(vp), C.POINTER(sz)]
    L.needle_hip_matcher_stats.argtypes = [vp, C.POINTER(u64)]
    L.needle_hip_crossmatcher_new.argtypes = [sz, sz, u32, u32, C.POINTER(vp)]
    L.needle_hip_crossmatcher_free.argtypes = [vp]
    L.needle_hip_crossmatcher_free.restype = None
    L.needle_hip_crossmatcher_feed.argtypes = [vp, C.POINTER(vp), C.POINTER(sz)]
    L.needle_hip_crossmatcher_feed_from_feeder.argtypes = [vp, vp]
    L.needle_hip_crossmatcher_finish.argtypes = [vp, C.POINTER(sz), sz]
    L.needle_hip_crossmatcher_ready.argtypes = [vp, C.POINTER(sz), C.POINTER(b)]
    L.needle_hip_crossmatcher_lane.argtypes = [vp, sz, C.POINTER(u64), C.POINTER(b)]
    L.needle_hip_crossmatcher_runs.argtypes = [vp, sz, sz, vp]
    L.needle_hip_crossmatcher_stats.argtypes = [vp, C.POINTER(u64)]
    L.needle_hip_crossmatcher_state_bytes.argtypes = [sz, sz]
    L.needle_hip_crossmatcher_state_bytes.restype = sz
    L.needle_hip_crossmatcher_new_regions.argtypes = [sz, sz, C.POINTER(sz), C.POINTER(u32), u32, C.POINTER(vp)]
    L.needle_hip_crossmatcher_state_bytes_regions.argtypes = [sz, sz, C.POINTER(sz)]
    L.needle_hip_crossmatcher_state_bytes_regions.restype = sz
    L.needle_hip_crossmatcher_shape.argtypes = [vp, C.POINTER(sz), C.POINTER(sz)]
    L.needle_hip_crossmatcher_new_resident.argtypes = [vp, sz, vp, sz, sz, sz, C.POINTER(sz), C.POINTER(u32), u32, C.POINTER(vp)]
    L.needle_hip_crossmatcher_state_bytes_resident.argtypes = [vp, sz, sz, sz, C.POINTER(sz)]
    L.needle_hip_crossmatcher_state_bytes_resident.restype = sz
    L.needle_hip_crossmatcher_resident.argtypes = [vp, C.POINTER(sz)]
    L.needle_hip_crossmatcher_new_grouped.argtypes = [vp, sz, vp, sz, vp, sz, vp, sz, C.POINTER(sz), C.POINTER(u32), u32, C.POINTER(vp)]
    L.needle_hip_crossmatcher_state_bytes_grouped.argtypes = [vp, sz, vp, sz, vp, sz, C.POINTER(sz)]
    L.needle_hip_crossmatcher_state_bytes_grouped.restype = sz
    L.needle_hip_crossmatcher_groups.argtypes = [vp, C.POINTER(u32), sz]
    _LIB = L
    return L


def check(code: int) -> None:
    if code != 0:
        raise NeedleError(code, (lib().needle_hip_last_error_message() or b"").decode(errors="replace"))


def error_to_str(code: int) -> str:
    return lib().needle_error_to_str(code).decode()


def device_count() -> int:
    n = C.c_int(0)
    check(lib().needle_hip_device_count(C.byref(n)))
    return n.value


def set_device(ordinal: int) -> None:
    check(lib().needle_hip_set_device(ordinal))


def device_pci_bus_id() -> str:
    buf = C.create_string_buffer(32)
    lib().needle_hip_device_pci_bus_id.argtypes = [C.c_char_p]
    check(lib().needle_hip_device_pci_bus_id(buf))
    return buf.value.decode()


def synchronize() -> None:
    check(lib().needle_hip_synchronize())


def stream_ptr() -> int:
    """The library's hipStream_t as an integer (e.g. for torch.cuda.ExternalStream)."""
    L = lib()
    L.needle_hip_stream.restype = C.c_void_p
    p = L.needle_hip_stream()
    if not p:
        raise RuntimeError("no HIP device: the library has no stream")
    return int(p)


def cert_stats(reset: bool = False) -> dict:
    """Counts of the certified f32 first pass (needle_hip_fingerprint_cert_stats)."""
    v = (C.c_uint64 * 4)()
    lib().needle_hip_fingerprint_cert_stats.argtypes = [C.POINTER(C.c_uint64), C.c_bool]
    check(lib().needle_hip_fingerprint_cert_stats(v, reset))
    return {"items": int(v[0]), "items_recomputed": int(v[1]), "chunks": int(v[2]), "chunks_recomputed": int(v[3])}


def scan_issued_evaluations(reset: bool = False) -> int:
    """Cell evaluations issued by the counting scan launches (NEEDLE_HIP_SCAN_COUNT=1) since the last reset."""
    v = C.c_uint64(0)
    lib().needle_hip_scan_issued_evaluations.argtypes = [C.POINTER(C.c_uint64), C.c_bool]
    check(lib().needle_hip_scan_issued_evaluations(C.byref(v), reset))
    return int(v.value)


def scan_counts(reset: bool = False) -> Tuple[int, int]:
    """(issued lane evaluations, diagonals that survived the head rows) of the counting scan launches."""
    c = (C.c_uint64 * 2)()
    lib().needle_hip_scan_counts.argtypes = [C.POINTER(C.c_uint64), C.c_bool]
    check(lib().needle_hip_scan_counts(c, reset))
    return int(c[0]), int(c[1])


def scan_last_launch() -> Tuple[int, int]:
    """(form, matrix products) of this process's last scan launch: form 3 = aligned windows on the vector ALU, 4 = with the
    head rows on the matrix pipe (then the second value counts its v_mfma_i32_32x32x32_i8 instructions)."""
    form, products = C.c_int32(0), C.c_uint64(0)
    lib().needle_hip_scan_last_launch.argtypes = [C.POINTER(C.c_int32), C.POINTER(C.c_uint64)]
    check(lib().needle_hip_scan_last_launch(C.byref(form), C.byref(products)))
    return int(form.value), int(products.value)


def epilogue_host_fallbacks(reset: bool = False) -> int:
    """Jobs whose device epilogue fell back to the host form (a pair's bucket of runs too large for one lane)."""
    jobs = C.c_uint64(0)
    lib().needle_hip_epilogue_host_fallbacks.argtypes = [C.POINTER(C.c_uint64), C.c_bool]
    check(lib().needle_hip_epilogue_host_fallbacks(C.byref(jobs), reset))
    return int(jobs.value)


def host_threads() -> int:
    """Host threads this process uses for its parallel host phases (needle_hip_host_threads)."""
    lib().needle_hip_host_threads.restype = C.c_int
    return int(lib().needle_hip_host_threads())


def int_valu_ceiling() -> float:
    """Measured cells/s of the scan's 4-instruction cell on registers (needle_hip_int_valu_ceiling)."""
    v = C.c_double(0.0)
    lib().needle_hip_int_valu_ceiling.argtypes = [C.POINTER(C.c_double)]
    check(lib().needle_hip_int_valu_ceiling(C.byref(v)))
    return v.value


def last_kernel_ms(name: str) -> float:
    return lib().needle_hip_last_kernel_ms(name.encode())


def kernel_launches(name: str) -> int:
    """Launches of that timer name since set_kernel_timing("...,sum") (needle_hip_kernel_launches)."""
    return int(lib().needle_hip_kernel_launches(name.encode()))


def set_kernel_timing(kernels: Optional[str]) -> None:
    """"all", a comma-separated list of kernel names, or None: which launches get HIP timing events."""
    lib().needle_hip_set_kernel_timing(kernels.encode() if kernels else None)


# ---- compressed fingerprints (chromaprint's codec, fp_codec.hip) ----------------------------------------
def _take_bytes(ptr, size: int) -> bytes:
    """The bytes of an array the library malloc'd, which is freed."""
    out = C.string_at(ptr, size) if size else b""
    lib().needle_hip_host_free(ptr)
    return out


def fingerprint_compressed_bound(items: int) -> int:
    """The most bytes a fingerprint of `items` items compresses to (pure host)."""
    return int(lib().needle_hip_fingerprint_compressed_bound(items))


def fingerprint_codec_tiles() -> Tuple[int, int]:
    """(items of a compress tile, 3-bit symbols of a decompress tile) of the device codec (pure host)."""
    t, d = C.c_size_t(), C.c_size_t()
    check(lib().needle_hip_fingerprint_codec_tiles(C.byref(t), C.byref(d)))
    return t.value, d.value


def fingerprint_base64_encode(data: bytes) -> str:
    text, size = C.c_void_p(), C.c_size_t()
    data = bytes(data)
    check(lib().needle_hip_fingerprint_base64_encode(data, len(data), C.byref(text), C.byref(size)))
    return _take_bytes(text, size.value).decode()


def fingerprint_base64_decode(text) -> bytes:
    raw = text.encode("latin-1") if isinstance(text, str) else bytes(text)
    data, size = C.c_void_p(), C.c_size_t()
    check(lib().needle_hip_fingerprint_base64_decode(raw, len(raw), C.byref(data), C.byref(size)))
    return _take_bytes(data, size.value)


def fingerprint_simhash(items) -> int:
    """chromaprint's 32-bit simhash of a fingerprint (pure host); 0 for an empty one."""
    arr = np.ascontiguousarray(items, dtype=np.uint32)
    h = C.c_uint32()
    check(lib().needle_hip_fingerprint_simhash(arr.ctypes.data if arr.size else None, arr.size, C.byref(h)))
    return h.value


def compress_fingerprints(fingerprints: Sequence, algorithm: int = 1, base64: bool = False) -> list:
    """Each fingerprint (uint32 items) in chromaprint's compressed form, on the device, all in one call: a list of bytes,
    or of base64 strings (URL-safe, unpadded: what fpcalc prints)."""
    arrays = [np.ascontiguousarray(f, dtype=np.uint32).ravel() for f in fingerprints]
    items = np.concatenate(arrays) if arrays else np.zeros(0, np.uint32)
    off = (C.c_uint64 * (len(arrays) + 1))(*np.concatenate([[0], np.cumsum([a.size for a in arrays])]).astype(np.uint64).tolist())
    blob_off = (C.c_uint64 * (len(arrays) + 1))()
    blobs = C.c_void_p()
    check(lib().needle_hip_fingerprint_compress_host(items.ctypes.data if items.size else None, off, len(arrays), algorithm,
                                                     C.byref(blobs), blob_off))
    data = _take_bytes(blobs, blob_off[len(arrays)])
    out = [data[blob_off[b]:blob_off[b + 1]] for b in range(len(arrays))]
    return [fingerprint_base64_encode(b) for b in out] if base64 else out


def decompress_fingerprints(blobs: Sequence, base64: bool = False):
    """(arrays, algorithms, status) of compressed fingerprints, on the device, all in one call.  status[b]: 0 ok, 1 shorter
    than a header, 2 the normal stream ends early, 3 the exceptional stream ends early, 4 a bit position above 32; a
    refused blob's array is empty.  base64: strings in; text that is not base64 raises NeedleError (InvalidArgument)."""
    raw = [fingerprint_base64_decode(b) if base64 else bytes(b) for b in blobs]
    data = b"".join(raw)
    off = (C.c_uint64 * (len(raw) + 1))(*np.concatenate([[0], np.cumsum([len(r) for r in raw])]).astype(np.uint64).tolist())
    item_off = (C.c_uint64 * (len(raw) + 1))()
    algorithms = np.zeros(max(len(raw), 1), np.int32)
    status = np.zeros(max(len(raw), 1), np.int32)
    items = C.c_void_p()
    check(lib().needle_hip_fingerprint_decompress_host(data if data else None, off, len(raw), C.byref(items), item_off,
                                                       algorithms.ctypes.data, status.ctypes.data))
    flat = np.frombuffer(_take_bytes(items, 4 * item_off[len(raw)]), dtype=np.uint32)
    arrays = [flat[item_off[b]:item_off[b + 1]].copy() for b in range(len(raw))]
    return arrays, algorithms[:len(raw)].tolist(), status[:len(raw)].tolist()


def _paths(paths: Sequence[str]):
    arr = (C.c_char_p * max(len(paths), 1))(*[p.encode() if isinstance(p, str) else p for p in paths])
    return C.cast(arr, C.POINTER(C.c_char_p)), arr


def header_md5(path: str) -> str:
    buf = C.create_string_buffer(33)
    check(lib().needle_hip_header_md5(path.encode(), buf))
    return buf.value.decode()


# ---- FrameHashes --------------------------------------------------------------------------------------
class FrameHashes:
    """needle::audio::FrameHashes (data.rs:74-168).  Wraps a library-owned or borrowed handle."""

    def __init__(self, handle: int, owned: bool, keepalive=None):
        self._h = C.c_void_p(handle)
        self._owned = owned
        self._keep = keepalive

    @staticmethod
    def new(opening: Sequence[Tuple[int, int]], ending: Sequence[Tuple[int, int]] = (), hash_duration_ns: int = 0,
            md5: str = "") -> "FrameHashes":
        oh = np.array([h for h, _ in opening], dtype=np.uint32)
        ot = np.array([t for _, t in opening], dtype=np.uint64)
        eh = np.array([h for h, _ in ending], dtype=np.uint32)
        et = np.array([t for _, t in ending], dtype=np.uint64)
        out = C.c_void_p()
        check(lib().needle_hip_frame_hashes_new(oh.ctypes.data, ot.ctypes.data, len(oh), eh.ctypes.data,
                                                et.ctypes.data, len(eh), hash_duration_ns, md5.encode(),
                                                C.byref(out)))
        return FrameHashes(out.value, True)

    @staticmethod
    def from_path(path: str) -> "FrameHashes":          # data.rs:104-115
        out = C.c_void_p()
        check(lib().needle_hip_frame_hashes_read(path.encode(), C.byref(out)))
        return FrameHashes(out.value, True)

    def write(self, path: str) -> None:
        check(lib().needle_hip_frame_hashes_write(self._h, path.encode()))

    def _data(self, ending: bool):
        n = lib().needle_hip_frame_hashes_len(self._h, ending)
        hashes = np.zeros(max(n, 1), dtype=np.uint32)
        ts = np.zeros(max(n, 1), dtype=np.uint64)
        check(lib().needle_hip_frame_hashes_copy(self._h, ending, hashes.ctypes.data, ts.ctypes.data, n))
        return hashes[:n], ts[:n]

    def opening_data(self):                              # data.rs:143
        return self._data(False)

    def ending_data(self):                               # data.rs:150
        return self._data(True)

    def hash_duration(self) -> int:                      # data.rs:157 (ns)
        return lib().needle_hip_frame_hashes_hash_duration_ns(self._h)

    def md5(self) -> str:                                # data.rs:164
        return lib().needle_hip_frame_hashes_md5(self._h).decode()

    def __del__(self):
        if getattr(self, "_owned", False) and self._h:
            lib().needle_hip_frame_hashes_free(self._h)
            self._h = None


@dataclass
class SearchResult:                                      # comparator.rs:65-69 (times in ns)
    opening: Optional[Tuple[int, int]]
    ending: Optional[Tuple[int, int]]


@dataclass
class MatchEvidence:                                     # NeedleHipMatchEvidence of a region that has a match
    partner: int
    is_source: bool
    candidate: int
    candidates: int
    support: int
    partners: int
    score: np.float32
    match_hash: int
    partner_hash: int
    interval: Tuple[int, int]                            # in this video, before padding (ns)
    partner_interval: Tuple[int, int]                    # the same run in the partner (ns)


@dataclass
class SearchEvidence:                                    # None: the region has no match
    opening: Optional[MatchEvidence]
    ending: Optional[MatchEvidence]


def _match_evidence(e) -> Optional[MatchEvidence]:
    if e.partner == NO_PARTNER:
        assert bytes(e)[4:] == bytes(C.sizeof(CMatchEvidence) - 4), "a region without a match: every other field is 0"
        return None
    assert e.reserved == 0
    return MatchEvidence(e.partner, bool(e.is_source), e.candidate, e.candidates, e.support, e.partners, np.float32(e.score),
                         e.match_hash, e.partner_hash, (e.start_ns, e.end_ns), (e.partner_start_ns, e.partner_end_ns))


def _evidence(arr, n) -> List[SearchEvidence]:
    return [SearchEvidence(_match_evidence(arr[i].opening), _match_evidence(arr[i].ending)) for i in range(n)]


def _results(arr, n) -> List[Optional[SearchResult]]:
    out: List[Optional[SearchResult]] = []
    for i in range(n):
        r = arr[i]
        if not r.has_result:
            out.append(None)
        else:
            out.append(SearchResult((r.opening_start_ns, r.opening_end_ns) if r.has_opening else None,
                                    (r.ending_start_ns, r.ending_end_ns) if r.has_ending else None))
    return out


# ---- Analyzer -------------------------------------------------------------------------------------------
class Analyzer:
    """needle::audio::Analyzer (analyzer.rs:86-151) over needle_audio_analyzer_* (needle-capi/src/lib.rs:354-491)."""

    def __init__(self, videos: Sequence[str], threaded_decoding: bool = False, force: bool = False,
                 opening_search_percentage: float = DEFAULT_OPENING_SEARCH_PERCENTAGE,
                 ending_search_percentage: float = DEFAULT_ENDING_SEARCH_PERCENTAGE, include_endings: bool = False):
        self.videos = list(videos)
        self._cfg = dict(opening=opening_search_percentage, ending=ending_search_percentage,
                         include_endings=include_endings, threaded=threaded_decoding, force=force)
        self._h = None
        self._mix: Optional[ChannelMix] = None
        self._layout_downmix = False

    @staticmethod
    def from_files(videos: Sequence[str], threaded_decoding: bool = False, force: bool = False) -> "Analyzer":
        return Analyzer(videos, threaded_decoding, force)

    def set_channel_mix(self, mix: Optional[ChannelMix]) -> "Analyzer":
        """run_pcm folds its `channels`-channel PCM with `mix` (needle_hip_analyzer_set_channel_mix; None: the plain
        average again).  The mix's limits are checked here; its channel count against the call's in run_pcm."""
        old, self._mix = self._mix, mix
        try:
            self._handle()
        except NeedleError:
            self._mix = old
            raise
        return self

    def set_layout_downmix(self, on: bool) -> "Analyzer":
        """run folds every WAV file that carries a channel mask with that mask's default mix
        (needle_hip_analyzer_set_layout_downmix); files without one keep the plain average."""
        self._layout_downmix = bool(on)
        return self

    def with_opening_search_percentage(self, v: float) -> "Analyzer":
        self._cfg["opening"] = v
        return self

    def with_ending_search_percentage(self, v: float) -> "Analyzer":
        self._cfg["ending"] = v
        return self

    def with_include_endings(self, v: bool) -> "Analyzer":
        self._cfg["include_endings"] = v
        return self

    def with_threaded_decoding(self, v: bool) -> "Analyzer":
        self._cfg["threaded"] = v
        return self

    def with_force(self, v: bool) -> "Analyzer":
        self._cfg["force"] = v
        return self

    def _handle(self):
        if self._h:
            lib().needle_audio_analyzer_free(self._h)
        ptr, keep = _paths(self.videos)
        out = C.c_void_p()
        c = self._cfg
        check(lib().needle_audio_analyzer_new(ptr, len(self.videos), c["opening"], c["ending"], c["include_endings"],
                                              c["threaded"], c["force"], C.byref(out)))
        self._h = out
        if self._mix is not None:
            check(lib().needle_hip_analyzer_set_channel_mix(out, C.byref(self._mix)))
        if self._layout_downmix:
            check(lib().needle_hip_analyzer_set_layout_downmix(out, True))
        return out

    def _collect(self) -> List[FrameHashes]:
        out = []
        for i in range(len(self.videos)):
            fh = C.c_void_p()
            check(lib().needle_audio_analyzer_get_frame_hashes(self._h, i, C.byref(fh)))
            out.append(FrameHashes(fh.value, False, keepalive=self))
        return out

    def run(self, hash_duration: float = DEFAULT_HASH_DURATION, persist: bool = False,
            threading: bool = True) -> List[FrameHashes]:          # analyzer.rs:425
        h = self._handle()
        check(lib().needle_audio_analyzer_run(h, hash_duration, persist, threading))
        return self._collect()

    def run_pcm(self, pcm: Sequence[np.ndarray], channels: int = 1, sample_rate: int = 11025,
                hash_duration: float = DEFAULT_HASH_DURATION, persist: bool = False,
                sample_format: int = SAMPLE_S16) -> List[FrameHashes]:
        """Same with decode already done: pcm[i] is the whole stream of video i (interleaved s16).  With another
        `sample_format` (SAMPLE_*) the samples go to the device as they are and are converted there
        (needle_hip_analyzer_run_pcm_format); a planar stream is a sequence of `channels` planes; num_values counts
        samples over all channels."""
        h = self._handle()
        if sample_format != SAMPLE_S16:
            keep, flat = _format_pointers(pcm, channels, sample_format)
            planar = sample_format_planar(sample_format)
            sizes = [sum(q.size for q in p) if planar else np.size(p) for p in pcm]
            ptrs = (C.c_void_p * max(len(flat), 1))(*flat)
            lens = (C.c_size_t * max(len(sizes), 1))(*sizes)
            check(lib().needle_hip_analyzer_run_pcm_format(h, ptrs, lens, channels, sample_rate, sample_format,
                                                           hash_duration, persist))
            del keep
            return self._collect()
        arrs = [np.ascontiguousarray(p, dtype=np.int16) for p in pcm]
        ptrs = (C.c_void_p * max(len(arrs), 1))(*[a.ctypes.data for a in arrs])
        lens = (C.c_size_t * max(len(arrs), 1))(*[a.size for a in arrs])
        check(lib().needle_hip_analyzer_run_pcm(h, ptrs, lens, channels, sample_rate, hash_duration, persist))
        return self._collect()

    def run_pcm_formats(self, pcm, formats: Sequence[Tuple[int, int, int]], mixes: Optional[Sequence[Optional[ChannelMix]]] = None,
                        hash_duration: float = DEFAULT_HASH_DURATION, persist: bool = False) -> List[FrameHashes]:
        """run_pcm with a (channels, sample_rate, sample_format) triple per stream and, optionally, a mix per stream
        (None: the plain average) in one device pass (needle_hip_analyzer_run_pcm_formats); a planar stream is a
        sequence of its planes."""
        h = self._handle()
        keep, flat, sizes = _lane_pointers(pcm, formats)
        ptrs = (C.c_void_p * max(len(flat), 1))(*flat)
        lens = (C.c_size_t * max(len(sizes), 1))(*sizes)
        check(lib().needle_hip_analyzer_run_pcm_formats(h, ptrs, lens, _lane_formats(formats),
                                                        None if mixes is None else _channel_mixes(mixes), hash_duration, persist))
        del keep
        return self._collect()

    def __del__(self):
        if getattr(self, "_h", None):
            lib().needle_audio_analyzer_free(self._h)
            self._h = None


# ---- Comparator ------------------------------------------------------------------------------------------
def _group_labels(groups: Sequence[int], n: int) -> np.ndarray:
    labels = np.ascontiguousarray(groups, dtype=np.uint32)
    if labels.shape != (n,):
        raise ValueError(f"{labels.size} group labels for {n} videos")
    return labels


def group_pairs(groups: Sequence[int]) -> np.ndarray:
    """The (a, b) of every grouped pair id in order, as an array of shape (pairs, 2) (needle_hip_group_pairs): what a
    grouped call searches, and how NeedleHipRun.problem // regions of its run list decodes."""
    labels = np.ascontiguousarray(groups, dtype=np.uint32)
    count = C.c_uint64(0)
    check(lib().needle_hip_group_pairs(labels.ctypes.data, labels.size, None, 0, C.byref(count)))
    pairs = np.zeros((count.value, 2), dtype=np.uint32)
    check(lib().needle_hip_group_pairs(labels.ctypes.data, labels.size, pairs.ctypes.data, count.value, C.byref(count)))
    return pairs


class Comparator:
    """needle::audio::Comparator (comparator.rs:74-147) over needle_audio_comparator_* (lib.rs:537-637)."""

    def __init__(self, videos: Sequence[str], include_endings: bool = False,
                 hash_match_threshold: int = DEFAULT_HASH_MATCH_THRESHOLD,
                 min_opening_duration: int = DEFAULT_MIN_OPENING_DURATION,
                 min_ending_duration: int = DEFAULT_MIN_ENDING_DURATION, time_padding: float = 0.0):
        self.videos = list(videos)
        self._cfg = dict(include_endings=include_endings, threshold=hash_match_threshold,
                         min_opening=min_opening_duration, min_ending=min_ending_duration, padding=time_padding)
        self._h = None

    @staticmethod
    def from_files(videos: Sequence[str]) -> "Comparator":
        return Comparator(videos)

    def with_include_endings(self, v: bool) -> "Comparator":
        self._cfg["include_endings"] = v
        return self

    def with_hash_match_threshold(self, v: int) -> "Comparator":
        self._cfg["threshold"] = v
        return self

    def with_min_opening_duration(self, secs: int) -> "Comparator":
        self._cfg["min_opening"] = secs
        return self

    def with_min_ending_duration(self, secs: int) -> "Comparator":
        self._cfg["min_ending"] = secs
        return self

    def with_time_padding(self, secs: float) -> "Comparator":
        self._cfg["padding"] = secs
        return self

    def handle(self):
        if self._h:
            lib().needle_audio_comparator_free(self._h)
        ptr, keep = _paths(self.videos)
        out = C.c_void_p()
        c = self._cfg
        check(lib().needle_audio_comparator_new(ptr, len(self.videos), c["include_endings"], c["threshold"],
                                                c["min_opening"], c["min_ending"], c["padding"], C.byref(out)))
        self._h = out
        return out

    def run_with_frame_hashes(self, frame_hashes: Sequence[FrameHashes], display: bool = False,
                              use_skip_files: bool = False, write_skip_files: bool = False,
                              groups: Optional[Sequence[int]] = None) -> List[Optional[SearchResult]]:       # comparator.rs:524
        """One entry per video; None where the reference pushes no result (comparator.rs:608-617).  groups: a label per
        video (any 32-bit value); only videos of equal label are compared (needle_hip.h "A library of many shows")."""
        h = self.handle()
        n = len(frame_hashes)
        ptrs = (C.c_void_p * max(n, 1))(*[f._h for f in frame_hashes])
        res = (CSearchResult * max(n, 1))()
        if groups is None:
            check(lib().needle_hip_comparator_run_with_frame_hashes(h, ptrs, n, display, use_skip_files,
                                                                    write_skip_files, res))
        else:
            labels = _group_labels(groups, n)
            check(lib().needle_hip_comparator_run_with_frame_hashes_grouped(h, ptrs, n, labels.ctypes.data, display,
                                                                            use_skip_files, write_skip_files, res))
        return _results(res, n)

    def results_from_runs_grouped(self, frame_hashes: Sequence[FrameHashes], groups: Sequence[int],
                                  runs: np.ndarray) -> List[Optional[SearchResult]]:
        """The host epilogue alone over a grouped run list (problem = grouped pair id * regions + region): no device work."""
        n = len(frame_hashes)
        runs = np.ascontiguousarray(runs, dtype=RUN_DTYPE)
        labels = _group_labels(groups, n)
        arr = (C.c_void_p * max(n, 1))(*[f._h for f in frame_hashes])
        res = (CSearchResult * max(n, 1))()
        check(lib().needle_hip_comparator_results_from_runs_grouped(self._h or self.handle(), arr, n, labels.ctypes.data,
                                                                    runs.ctypes.data, runs.size, res))
        return _results(res, n)

    def results_from_runs(self, frame_hashes: Sequence[FrameHashes], runs: np.ndarray, first_video: int = 0,
                          video_count: Optional[int] = None) -> List[Optional[SearchResult]]:
        """The host epilogue alone (needle_hip_comparator_results_from_runs): no device work."""
        n = len(frame_hashes)
        runs = np.ascontiguousarray(runs, dtype=RUN_DTYPE)
        arr = (C.c_void_p * max(n, 1))(*[f._h for f in frame_hashes])
        res = (CSearchResult * max(n, 1))()
        check(lib().needle_hip_comparator_results_from_runs(
            self._h or self.handle(), arr, n, runs.ctypes.data, runs.size, first_video,
            n - first_video if video_count is None else video_count, res))
        return _results(res, n)

    def results_from_runs_evidence(self, frame_hashes: Sequence[FrameHashes], runs: np.ndarray, first_video: int = 0,
                                   video_count: Optional[int] = None) -> Tuple[List[Optional[SearchResult]], List[SearchEvidence]]:
        """results_from_runs with the evidence beside every result (needle_hip_comparator_results_from_runs_evidence)."""
        n = len(frame_hashes)
        runs = np.ascontiguousarray(runs, dtype=RUN_DTYPE)
        arr = (C.c_void_p * max(n, 1))(*[f._h for f in frame_hashes])
        res = (CSearchResult * max(n, 1))()
        ev = (CSearchEvidence * max(n, 1))()
        check(lib().needle_hip_comparator_results_from_runs_evidence(
            self._h or self.handle(), arr, n, runs.ctypes.data, runs.size, first_video,
            n - first_video if video_count is None else video_count, res, ev))
        return _results(res, n), _evidence(ev, n)

    def run(self, analyze: bool, display: bool = False, use_skip_files: bool = False,
            write_skip_files: bool = False, threading: bool = True, groups: Optional[Sequence[int]] = None) -> None:   # comparator.rs:637 / lib.rs:612
        h = self.handle()
        if groups is None:
            check(lib().needle_audio_comparator_run(h, analyze, display, use_skip_files, write_skip_files, threading))
        else:  # a label per path
            labels = np.ascontiguousarray(groups, dtype=np.uint32)
            check(lib().needle_hip_comparator_run_grouped(h, labels.ctypes.data, labels.size, analyze, display, use_skip_files,
                                                          write_skip_files))

    def __del__(self):
        if getattr(self, "_h", None):
            lib().needle_audio_comparator_free(self._h)
            self._h = None


class Index:
    """An incremental search index (needle_hip_index_*): results() equals Comparator.run_with_frame_hashes over the
    index's current list of videos; add() searches only the pairs it adds, remove() none, replace() those of the videos
    replaced.  The comparator's parameters are copied at
    creation.  One GPU: the device current at creation.
    grouped=True: a library of many seasons (needle_hip_index_new_grouped) -- every video is added with a label, equal
    labels are one season, only pairs inside a season are searched, and results() equals
    Comparator.run_with_frame_hashes(groups=...) over the current list."""

    def __init__(self, comparator: Comparator, grouped: bool = False):
        self._h = None
        out = C.c_void_p()
        new = lib().needle_hip_index_new_grouped if grouped else lib().needle_hip_index_new
        check(new(comparator.handle(), C.byref(out)))
        self._h = out
        self.grouped = bool(grouped)
        self.threshold = comparator._cfg["threshold"]   # copied, as the index copies it
        self.include_endings = bool(comparator._cfg["include_endings"])

    def add(self, frame_hashes: Sequence[FrameHashes], groups: Optional[Sequence[int]] = None) -> None:
        """Appends the videos; on failure (NeedleError) the index is as it was before the call.  groups: a label per
        video (0 .. 2^32 - 1, only compared), for a grouped index -- which refuses an add without them, as a plain index
        refuses one with them."""
        k = len(frame_hashes)
        ptrs = (C.c_void_p * max(k, 1))(*[f._h for f in frame_hashes])
        if groups is None:
            check(lib().needle_hip_index_add(self._h, ptrs, k))
            return
        if len(groups) != k:
            raise ValueError("add: one group label per video")
        labels = (C.c_uint32 * max(k, 1))(*[int(g) for g in groups])
        check(lib().needle_hip_index_add_grouped(self._h, ptrs, labels, k))

    def groups(self) -> List[int]:
        """The current list's labels, one per video (a grouped index; a plain one: NeedleError)."""
        n = len(self)
        labels = (C.c_uint32 * max(n, 1))()
        check(lib().needle_hip_index_groups(self._h, labels, n))
        return list(labels[:n])

    def remove(self, positions: Sequence[int]) -> None:
        """Removes the videos at these distinct positions; the others keep their order.  On failure (NeedleError) the
        index is as it was before the call."""
        k = len(positions)
        pos = (C.c_size_t * max(k, 1))(*positions)
        check(lib().needle_hip_index_remove(self._h, pos, C.c_size_t(k)))

    def replace(self, positions: Sequence[int], frame_hashes: Sequence[FrameHashes]) -> None:
        """Replaces the video at positions[i] with frame_hashes[i], in place; searches only the pairs of those videos."""
        k = len(positions)
        if len(frame_hashes) != k:
            raise ValueError("replace: one FrameHashes per position")
        pos = (C.c_size_t * max(k, 1))(*positions)
        ptrs = (C.c_void_p * max(k, 1))(*[f._h for f in frame_hashes])
        check(lib().needle_hip_index_replace(self._h, pos, ptrs, C.c_size_t(k)))

    def crossmatcher(self, videos: int, max_items: Sequence[int], min_len: Sequence[int],
                     groups: Optional[Sequence[int]] = None) -> "CrossMatcher":
        """A CrossMatcher whose resident videos are this index's (their rows copied from the index's device arena) with
        `videos` arriving ones; one max_items and one min_len per region of the index.  Feed it, then add_matched.
        `groups` (a grouped index): the arriving videos' labels; the residents carry the index's, and only same-label pairs
        are live.  Without `groups` a grouped index refuses."""
        if len(max_items) != len(min_len):
            raise ValueError(f"one max_items and one min_len per region: {len(max_items)} and {len(min_len)}")
        regions = len(max_items)
        h = C.c_void_p()
        if groups is not None:
            if len(groups) != videos:
                raise ValueError(f"one label per arriving video: {videos}, got {len(groups)}")
            check(lib().needle_hip_index_crossmatcher_new_grouped(self._h, videos, (C.c_uint32 * max(videos, 1))(*groups),
                                                                  (C.c_size_t * max(regions, 1))(*max_items),
                                                                  (C.c_uint32 * max(regions, 1))(*min_len), C.byref(h)))
        else:
            check(lib().needle_hip_index_crossmatcher_new(self._h, videos, (C.c_size_t * max(regions, 1))(*max_items),
                                                          (C.c_uint32 * max(regions, 1))(*min_len), C.byref(h)))
        m = CrossMatcher.__new__(CrossMatcher)
        m._h = h
        m._grouped = groups is not None
        videos, regions = m.shape()
        m.lanes, m.max_items, m.min_len, m.threshold = videos * regions, tuple(max_items), tuple(min_len), self.threshold
        return m

    def add_matched(self, matcher: "CrossMatcher", frame_hashes: Sequence[FrameHashes]) -> None:
        """Appends the matcher's arriving videos (complete, made by crossmatcher() since the last change) with the runs it
        holds in place of a scan; afterwards the index is what add(frame_hashes) leaves.  On failure (NeedleError) the
        index is as it was before the call.  A matcher with groups (crossmatcher(groups=...)) goes to
        needle_hip_index_add_matched_grouped: the videos are appended under the matcher's labels, as add(groups=...) would."""
        k = len(frame_hashes)
        ptrs = (C.c_void_p * max(k, 1))(*[f._h for f in frame_hashes])
        if getattr(matcher, "_grouped", False):
            check(lib().needle_hip_index_add_matched_grouped(self._h, matcher._h, ptrs, k))
        else:
            check(lib().needle_hip_index_add_matched(self._h, matcher._h, ptrs, k))

    def matcher(self, videos: int) -> "Matcher":
        """A Matcher whose sources are this index's rows (gathered from the index's device arena; min_len per row, the
        index's regions and threshold) with `videos * regions` lanes: the resident x arriving half of a streamed season, at
        any library size.  Feed it and a CrossMatcher.with_regions over the same videos, then add_streamed."""
        h = C.c_void_p()
        check(lib().needle_hip_index_matcher_new(self._h, videos, C.byref(h)))
        m = Matcher.__new__(Matcher)
        m._h = h
        m.regions = 2 if self.include_endings else 1
        m.lanes, m.num_sources, m.threshold = videos * m.regions, len(self) * m.regions, self.threshold
        return m

    def add_streamed(self, matcher: "Matcher", crossmatcher: Optional["CrossMatcher"], frame_hashes: Sequence[FrameHashes]) -> None:
        """Appends the arriving videos with the runs of `matcher` (complete, made by matcher() since the last change) for
        the resident x arriving pairs and those of `crossmatcher` (complete, no residents, over the same videos; None with
        one video) for the arriving pairs, in place of a scan; afterwards the index is what add(frame_hashes) leaves.  On
        failure (NeedleError) the index is as it was before the call."""
        k = len(frame_hashes)
        ptrs = (C.c_void_p * max(k, 1))(*[f._h for f in frame_hashes])
        check(lib().needle_hip_index_add_streamed(self._h, matcher._h, None if crossmatcher is None else crossmatcher._h, ptrs, k))

    def pairs_scanned(self) -> Tuple[int, int]:
        """(total, last): video pairs handed to the one-shot scan over the index's life and by the last operation (0 after
        add_matched and add_streamed)."""
        total, last = C.c_uint64(), C.c_uint64()
        check(lib().needle_hip_index_pairs_scanned(self._h, C.byref(total), C.byref(last)))
        return total.value, last.value

    def store_sizes(self) -> Tuple[int, int, int, int]:
        """(heap entries held, entry slots in use, hashes in the device arena, timestamps in the device table)."""
        sizes = (C.c_uint64 * 4)()
        check(lib().needle_hip_index_store_sizes(self._h, sizes))
        return tuple(int(x) for x in sizes)

    def results(self) -> List[Optional[SearchResult]]:
        n = len(self)
        res = (CSearchResult * max(n, 1))()
        check(lib().needle_hip_index_results(self._h, res, n))
        return _results(res, n)

    def evidence(self) -> List[SearchEvidence]:
        """Why every video got its result (needle_hip_index_evidence): computed on the device when asked, from the
        committed store; partners are current positions.  Changes nothing."""
        n = len(self)
        ev = (CSearchEvidence * max(n, 1))()
        check(lib().needle_hip_index_evidence(self._h, ev, n))
        return _evidence(ev, n)

    def pairs_searched(self) -> Tuple[int, int]:
        """(total, last): video pairs that entered the index over its life and by the last add."""
        total, last = C.c_uint64(), C.c_uint64()
        check(lib().needle_hip_index_pairs_searched(self._h, C.byref(total), C.byref(last)))
        return total.value, last.value

    def __len__(self) -> int:
        return int(lib().needle_hip_index_len(self._h))

    def __del__(self):
        if getattr(self, "_h", None):
            lib().needle_hip_index_free(self._h)
            self._h = None


# ---- kernel-level entry points ------------------------------------------------------------------------------
def feeder_num_ready(samples_per_channel_fed: int, sample_rate: int = 11025, channels: int = 1, step: int = 1,
                     finished: bool = False) -> int:
    """Kept items a Feeder lane holds after that many samples (host arithmetic, no device)."""
    return int(lib().needle_hip_feeder_num_ready(samples_per_channel_fed, sample_rate, channels, step, finished))


def _segments(segments):
    """NeedleHipSegment array of ((channels, sample_rate, sample_format), frames) pairs."""
    arr = (CSegment * max(len(segments), 1))()
    for i, ((c, r, f), frames) in enumerate(segments):
        arr[i].format = CLaneFormat(int(c), int(r), int(f))
        arr[i].frames = int(frames)
    return arr


def num_ready_segments(segments: Sequence[Tuple[Tuple[int, int, int], int]], step: int = 1, finished: bool = False) -> int:
    """Kept items a Feeder lane holds after these segments, ((channels, sample_rate, sample_format), frames) each, the
    last one open unless finished (needle_hip_feeder_num_ready_segments: host arithmetic, no device)."""
    return int(lib().needle_hip_feeder_num_ready_segments(_segments(segments), len(segments), step, finished))


class Feeder:
    """needle_hip_feeder_*: chromaprint's start / feed / finish batched over `lanes`, state on the device."""

    NO_LANE = C.c_size_t(-1).value  # SIZE_MAX: no ending lane

    def __init__(self, lanes: int, channels: int = 1, sample_rate: int = 11025, sample_format: int = SAMPLE_S16,
                 step: int = 1):
        self._h = None
        h = C.c_void_p()
        check(lib().needle_hip_feeder_new(lanes, channels, sample_rate, sample_format, step, C.byref(h)))
        self._h = h
        self.lanes, self.channels, self.sample_rate, self.sample_format, self.step = lanes, channels, sample_rate, sample_format, step
        self.formats = None

    @classmethod
    def with_formats(cls, formats: Sequence[Tuple[int, int, int]], step: int = 1) -> "Feeder":
        """needle_hip_feeder_new_lanes: one lane per (channels, sample_rate, sample_format) triple.  Every lane is
        down-mixed to mono as it lands; the items are the one-shot path's."""
        self = cls.__new__(cls)
        self._h = None
        formats = [tuple(int(v) for v in f) for f in formats]
        h = C.c_void_p()
        check(lib().needle_hip_feeder_new_lanes(_lane_formats(formats), len(formats), step, C.byref(h)))
        self._h = h
        self.lanes, self.step, self.formats = len(formats), step, formats
        self.channels = self.sample_rate = self.sample_format = None  # per lane: lane_format
        return self

    def lane_format(self, lane: int) -> Tuple[int, int, int]:
        """(channels, sample_rate, sample_format) of a lane, of either kind of feeder."""
        f = CLaneFormat()
        check(lib().needle_hip_feeder_lane_format(self._h, lane, C.byref(f)))
        return f.channels, f.sample_rate, f.format

    def set_lane_mix(self, lanes: Sequence[int], mixes: Sequence[Optional[ChannelMix]]) -> None:
        """lanes[j] folds its channels with mixes[j] (None: the plain average again); a with_formats feeder only, and only
        lanes that hold no samples (needle_hip_feeder_set_lane_mix)."""
        if len(lanes) != len(mixes):
            raise ValueError("one mix (or None) per lane")
        k = len(lanes)
        arr = (C.c_size_t * max(k, 1))(*lanes)
        check(lib().needle_hip_feeder_set_lane_mix(self._h, arr, _channel_mixes(mixes), k))

    def reset_format(self, lanes: Sequence[int], formats: Sequence[Tuple[int, int, int]]) -> None:
        """lanes[j] starts a new stream in formats[j] (needle_hip_feeder_reset_format; a with_formats feeder only)."""
        if len(lanes) != len(formats):
            raise ValueError("one format per lane")
        arr, k = self._lanes(list(lanes))
        check(lib().needle_hip_feeder_reset_format(self._h, arr, _lane_formats(formats), k))
        for lane, f in zip(lanes, formats):
            self.formats[lane] = tuple(int(v) for v in f)

    def switch_format(self, lanes: Sequence[int], formats: Sequence[Tuple[int, int, int]],
                      mixes: Optional[Sequence[Optional[ChannelMix]]] = None) -> None:
        """lanes[j] ends its current segment and continues ITS SAME STREAM in formats[j], folded by mixes[j] (None: the
        plain average) -- a decoder that reports another rate, layout or sample format in mid-stream
        (needle_hip_feeder_switch_format; a with_formats feeder only)."""
        if len(lanes) != len(formats) or (mixes is not None and len(mixes) != len(lanes)):
            raise ValueError("one format (and one mix or None) per lane")
        arr, k = self._lanes(list(lanes))
        check(lib().needle_hip_feeder_switch_format(self._h, arr, _lane_formats(formats), None if mixes is None else _channel_mixes(mixes), k))
        for lane, f in zip(lanes, formats):   # (a Feeder(...) of one format has been refused above)
            self.formats[lane] = tuple(int(v) for v in f)

    def lane_segments(self, lane: int) -> List[Tuple[Tuple[int, int, int], int]]:
        """The segments of the lane's current stream, ((channels, sample_rate, sample_format), frames) each, the open one
        last (needle_hip_feeder_lane_segments)."""
        count = C.c_size_t()
        check(lib().needle_hip_feeder_lane_segments(self._h, lane, None, 0, C.byref(count)))
        arr = (CSegment * max(count.value, 1))()
        check(lib().needle_hip_feeder_lane_segments(self._h, lane, arr, count.value, C.byref(count)))
        return [((s.format.channels, s.format.sample_rate, s.format.format), int(s.frames)) for s in arr[:count.value]]

    def feed(self, pcm: Sequence) -> None:
        """pcm[i]: what lane i has decoded since the last feed (interleaved: one array; planar: `channels` planes), or
        None / an empty array for nothing."""
        if len(pcm) != self.lanes:
            raise ValueError(f"one chunk per lane: {self.lanes}, got {len(pcm)}")
        if self.formats is not None:
            keep, flat, sizes = _lane_pointers(pcm, self.formats)
        else:
            planar = sample_format_planar(self.sample_format)
            keep, flat = _format_pointers(pcm, self.channels, self.sample_format)
            sizes = [0 if p is None else (sum(np.size(q) for q in p) if planar else np.size(p)) for p in pcm]
        ptrs = (C.c_void_p * max(len(flat), 1))(*flat)
        lens = (C.c_size_t * max(len(sizes), 1))(*sizes)
        check(lib().needle_hip_feeder_feed(self._h, ptrs, lens))
        del keep

    def _lanes(self, lanes):
        if lanes is None:
            return None, 0
        return (C.c_size_t * max(len(lanes), 1))(*lanes), len(lanes)

    def finish(self, lanes: Optional[Sequence[int]] = None) -> None:
        arr, k = self._lanes(lanes)
        check(lib().needle_hip_feeder_finish(self._h, arr, k))

    def reset(self, lanes: Optional[Sequence[int]] = None) -> None:
        arr, k = self._lanes(lanes)
        check(lib().needle_hip_feeder_reset(self._h, arr, k))

    def ready(self, lane: int) -> Tuple[int, int, bool]:
        """(kept items, samples per channel fed, finished) of a lane; waits for outstanding device work."""
        kept, fed, fin = C.c_size_t(), C.c_uint64(), C.c_bool()
        check(lib().needle_hip_feeder_ready(self._h, lane, C.byref(kept), C.byref(fed), C.byref(fin)))
        return kept.value, fed.value, fin.value

    def items(self, lane: int, first: int = 0, count: Optional[int] = None) -> np.ndarray:
        if count is None:
            count = self.ready(lane)[0] - first
        out = np.zeros(max(count, 0), dtype=np.uint32)
        check(lib().needle_hip_feeder_items(self._h, lane, first, count, out.ctypes.data if count else None))
        return out

    def compressed(self, lane: int, algorithm: int = 1, base64: bool = False):
        """A finished lane's kept items in chromaprint's compressed form (bytes, or the base64 string fpcalc prints)."""
        blob, size = C.c_void_p(), C.c_size_t()
        check(lib().needle_hip_feeder_compressed(self._h, lane, algorithm, C.byref(blob), C.byref(size)))
        data = _take_bytes(blob, size.value)
        return fingerprint_base64_encode(data) if base64 else data

    def frame_hashes(self, opening_lane: int, ending_lane: Optional[int] = None, ending_seek_ns: int = 0,
                     hash_duration: float = DEFAULT_HASH_DURATION, md5: str = "") -> "FrameHashes":
        h = C.c_void_p()
        check(lib().needle_hip_feeder_frame_hashes(self._h, opening_lane, self.NO_LANE if ending_lane is None else ending_lane,
                                                   ending_seek_ns, hash_duration, md5.encode(), C.byref(h)))
        return FrameHashes(h.value, True)

    def state_bytes(self) -> Tuple[int, int]:
        """(the most bytes one lane has carried from one feed to the next, high-water of one feed's staging)"""
        out = (C.c_uint64 * 2)()
        check(lib().needle_hip_feeder_state_bytes(self._h, out))
        return int(out[0]), int(out[1])

    def set_audit(self, on: bool) -> None:
        """Switches the audit that travels with the stream (needle_hip_feeder_set_audit); only while no lane holds samples."""
        check(lib().needle_hip_feeder_set_audit(self._h, bool(on)))

    def audit(self, lane: Optional[int] = None) -> dict:
        """The audit of a lane's current stream so far, or of all lanes (None: counts summed, maxima taken), as
        Library.audit (needle_hip_feeder_audit); waits for outstanding device work."""
        a = CCertAudit()
        check(lib().needle_hip_feeder_audit(self._h, self.NO_LANE if lane is None else lane, C.byref(a)))
        return a.as_dict()

    def __del__(self):
        if getattr(self, "_h", None):
            lib().needle_hip_feeder_free(self._h)
            self._h = None


class Matcher:
    """needle_hip_matcher_*: the streaming comparator.  `sources` (hash sequences, resident on the device from here on)
    against `lanes` destination sequences that arrive in chunks; run lists are RUN_DTYPE arrays, `problem` = the source."""

    def __init__(self, sources: Sequence[np.ndarray], min_len: Sequence[int], lanes: int, threshold: int):
        self._h = None
        arrs = [np.ascontiguousarray(s, dtype=np.uint32) for s in sources]
        arena = np.concatenate(arrs) if arrs else np.zeros(0, dtype=np.uint32)
        seqs = np.zeros((max(len(arrs), 1), 2), dtype=np.uint32)
        seqs[:len(arrs), 1] = [a.size for a in arrs]
        seqs[:len(arrs), 0] = np.cumsum([0] + [a.size for a in arrs])[:len(arrs)]
        mins = np.ascontiguousarray(list(min_len) or [0], dtype=np.uint32)
        if len(min_len) != len(arrs):
            raise ValueError("one min_len per source")
        h = C.c_void_p()
        check(lib().needle_hip_matcher_new(arena.ctypes.data if arena.size else None, arena.size, seqs.ctypes.data, mins.ctypes.data,
                                           len(arrs), lanes, threshold, C.byref(h)))
        self._h = h
        self.lanes, self.num_sources, self.threshold, self.regions = lanes, len(arrs), threshold, 1

    @classmethod
    def with_regions(cls, sources: Sequence[np.ndarray], min_len: Sequence[int], regions: int, lanes: int,
                     threshold: int) -> "Matcher":
        """needle_hip_matcher_new_regions: source s is in region s % regions, lane l in region l % regions, and a lane meets
        its own region's sources only; `problem` stays the source's index.  A min_len of 0 is allowed: that source has no
        cells."""
        arrs = [np.ascontiguousarray(s, dtype=np.uint32) for s in sources]
        if len(min_len) != len(arrs):
            raise ValueError("one min_len per source")
        arena = np.concatenate(arrs) if arrs else np.zeros(0, dtype=np.uint32)
        seqs = np.zeros((max(len(arrs), 1), 2), dtype=np.uint32)
        seqs[:len(arrs), 1] = [a.size for a in arrs]
        seqs[:len(arrs), 0] = np.cumsum([0] + [a.size for a in arrs])[:len(arrs)]
        mins = np.ascontiguousarray(list(min_len) or [0], dtype=np.uint32)
        self = cls.__new__(cls)
        self._h = None
        h = C.c_void_p()
        check(lib().needle_hip_matcher_new_regions(arena.ctypes.data if arena.size else None, arena.size, seqs.ctypes.data,
                                                   mins.ctypes.data, len(arrs), regions, lanes, threshold, C.byref(h)))
        self._h = h
        self.lanes, self.num_sources, self.threshold, self.regions = lanes, len(arrs), threshold, regions
        return self

    def feed(self, items: Sequence) -> None:
        """items[i]: the hashes lane i has received since the last feed, or None / an empty array for nothing."""
        if len(items) != self.lanes:
            raise ValueError(f"one chunk per lane: {self.lanes}, got {len(items)}")
        keep = [None if a is None else np.ascontiguousarray(a, dtype=np.uint32) for a in items]
        ptrs = (C.c_void_p * self.lanes)(*[None if a is None or a.size == 0 else a.ctypes.data for a in keep])
        lens = (C.c_size_t * self.lanes)(*[0 if a is None else a.size for a in keep])
        check(lib().needle_hip_matcher_feed(self._h, ptrs, lens))
        del keep

    def feed_from_feeder(self, feeder: "Feeder") -> None:
        """Takes, lane by lane, the feeder's ready items this matcher has not yet taken; finishes the lanes it has finished."""
        check(lib().needle_hip_matcher_feed_from_feeder(self._h, feeder._h))

    def _lanes(self, lanes):
        if lanes is None:
            return None, 0
        return (C.c_size_t * max(len(lanes), 1))(*lanes), len(lanes)

    def finish(self, lanes: Optional[Sequence[int]] = None) -> None:
        arr, k = self._lanes(lanes)
        check(lib().needle_hip_matcher_finish(self._h, arr, k))

    def reset(self, lanes: Optional[Sequence[int]] = None) -> None:
        arr, k = self._lanes(lanes)
        check(lib().needle_hip_matcher_reset(self._h, arr, k))

    def ready(self, lane: int) -> Tuple[int, int, bool]:
        """(runs reported, items fed, finished) of a lane."""
        runs, fed, fin = C.c_size_t(), C.c_uint64(), C.c_bool()
        check(lib().needle_hip_matcher_ready(self._h, lane, C.byref(runs), C.byref(fed), C.byref(fin)))
        return runs.value, fed.value, fin.value

    def runs(self, lane: int, first: int = 0, count: Optional[int] = None) -> np.ndarray:
        if count is None:
            count = self.ready(lane)[0] - first
        out = np.zeros(max(count, 0), dtype=RUN_DTYPE)
        check(lib().needle_hip_matcher_runs(self._h, lane, first, count, out.ctypes.data if count else None))
        return out

    def open(self, lane: int) -> np.ndarray:
        """The runs still open at the last column fed whose length is already >= min_len (simhash fields zero)."""
        ptr, n = C.c_void_p(), C.c_size_t()
        check(lib().needle_hip_matcher_open(self._h, lane, C.byref(ptr), C.byref(n)))
        try:
            return np.frombuffer(C.string_at(ptr.value, n.value * RUN_DTYPE.itemsize), dtype=RUN_DTYPE).copy()
        finally:
            lib().needle_hip_host_free(ptr)

    def stats(self) -> Tuple[int, int, int, int]:
        """(feeds, kernel launches, cells evaluated, bytes of state on the device)"""
        out = (C.c_uint64 * 4)()
        check(lib().needle_hip_matcher_stats(self._h, out))
        return tuple(int(x) for x in out)

    def __del__(self):
        if getattr(self, "_h", None):
            lib().needle_hip_matcher_free(self._h)
            self._h = None


class CrossMatcher:
    """needle_hip_crossmatcher_*: the streaming all-pairs comparator.  `lanes` sequences of at most `max_items` hashes arrive
    in chunks and are matched against each other; the run list is one RUN_DTYPE array, `problem` = the pair's index in the
    comparator's i-major order, so it goes straight into Comparator.results_from_runs.  `with_regions`: openings and endings
    in one object, lane = video * regions + region, `problem` = pair * regions + region.  `with_resident`: K known videos in
    front of the arriving ones; only the arriving videos have lanes, `problem` numbers the pairs over all K + N videos, and
    the list goes into Comparator.results_from_runs(first_video=K).  `with_groups`: a label per video, only same-label pairs
    with an arriving end are live, `problem` = grouped pair id * regions + region (Comparator.results_from_runs_grouped)."""

    def __init__(self, lanes: int, max_items: int, min_len: int, threshold: int):
        self._h = None
        h = C.c_void_p()
        check(lib().needle_hip_crossmatcher_new(lanes, max_items, min_len, threshold, C.byref(h)))
        self._h = h
        self.lanes, self.max_items, self.min_len, self.threshold = lanes, max_items, min_len, threshold

    @classmethod
    def with_regions(cls, videos: int, max_items: Sequence[int], min_len: Sequence[int], threshold: int) -> "CrossMatcher":
        """`videos * len(max_items)` lanes; max_items[r] and min_len[r] are region r's capacity and shortest run."""
        if len(max_items) != len(min_len):
            raise ValueError(f"one max_items and one min_len per region: {len(max_items)} and {len(min_len)}")
        regions = len(max_items)
        self = cls.__new__(cls)
        self._h = None
        h = C.c_void_p()
        check(lib().needle_hip_crossmatcher_new_regions(videos, regions, (C.c_size_t * max(regions, 1))(*max_items),
                                                        (C.c_uint32 * max(regions, 1))(*min_len), threshold, C.byref(h)))
        self._h = h
        self.lanes, self.max_items, self.min_len, self.threshold = videos * regions, tuple(max_items), tuple(min_len), threshold
        return self

    @classmethod
    def with_resident(cls, resident: Sequence[np.ndarray], videos: int, max_items: Sequence[int], min_len: Sequence[int],
                      threshold: int) -> "CrossMatcher":
        """`resident`: the K * regions hash sequences of the known videos in row order (video k, region r at k * regions + r),
        regions = len(max_items); `videos` arriving videos with `videos * regions` lanes."""
        if len(max_items) != len(min_len):
            raise ValueError(f"one max_items and one min_len per region: {len(max_items)} and {len(min_len)}")
        regions = len(max_items)
        if regions and len(resident) % regions:
            raise ValueError(f"one resident row per video and region: {len(resident)} rows, {regions} regions")
        arrs = [np.ascontiguousarray(s, dtype=np.uint32) for s in resident]
        arena = np.concatenate(arrs) if arrs else np.zeros(0, dtype=np.uint32)
        seqs = np.zeros((max(len(arrs), 1), 2), dtype=np.uint32)
        seqs[:len(arrs), 1] = [a.size for a in arrs]
        seqs[:len(arrs), 0] = np.cumsum([0] + [a.size for a in arrs])[:len(arrs)]
        self = cls.__new__(cls)
        self._h = None
        h = C.c_void_p()
        check(lib().needle_hip_crossmatcher_new_resident(arena.ctypes.data if arena.size else None, arena.size, seqs.ctypes.data,
                                                         len(arrs) // max(regions, 1), videos, regions,
                                                         (C.c_size_t * max(regions, 1))(*max_items),
                                                         (C.c_uint32 * max(regions, 1))(*min_len), threshold, C.byref(h)))
        self._h = h
        self.lanes, self.max_items, self.min_len, self.threshold = videos * regions, tuple(max_items), tuple(min_len), threshold
        return self

    @staticmethod
    def _rows(resident: Sequence[np.ndarray]):
        arrs = [np.ascontiguousarray(s, dtype=np.uint32) for s in resident]
        arena = np.concatenate(arrs) if arrs else np.zeros(0, dtype=np.uint32)
        seqs = np.zeros((max(len(arrs), 1), 2), dtype=np.uint32)
        seqs[:len(arrs), 1] = [a.size for a in arrs]
        seqs[:len(arrs), 0] = np.cumsum([0] + [a.size for a in arrs])[:len(arrs)]
        return arrs, arena, seqs

    @classmethod
    def with_groups(cls, groups: Sequence[int], max_items: Sequence[int], min_len: Sequence[int], threshold: int,
                    videos: Optional[int] = None, resident: Sequence[np.ndarray] = (),
                    resident_groups: Sequence[int] = ()) -> "CrossMatcher":
        """Groups of videos: groups[t] is the label of arriving video t (`videos` = len(groups) of them, `videos * regions`
        lanes), resident_groups[k] that of resident k, whose rows are `resident` as in with_resident.  Only same-label pairs
        with an arriving end are live; `problem` = (grouped pair id over all K + N labels) * regions + region, the numbering
        group_pairs() decodes, so without residents the list goes into Comparator.results_from_runs_grouped."""
        if len(max_items) != len(min_len):
            raise ValueError(f"one max_items and one min_len per region: {len(max_items)} and {len(min_len)}")
        regions = len(max_items)
        videos = len(groups) if videos is None else videos
        if videos != len(groups):
            raise ValueError(f"one label per arriving video: {videos}, got {len(groups)}")
        if len(resident) != len(resident_groups) * regions:
            raise ValueError(f"one resident row per video and region: {len(resident)} rows, {len(resident_groups)} labels, {regions} regions")
        arrs, arena, seqs = cls._rows(resident)
        labels = np.ascontiguousarray(groups, dtype=np.uint32)
        res_labels = np.ascontiguousarray(resident_groups, dtype=np.uint32)
        self = cls.__new__(cls)
        self._h = None
        h = C.c_void_p()
        check(lib().needle_hip_crossmatcher_new_grouped(arena.ctypes.data if arena.size else None, arena.size,
                                                        seqs.ctypes.data if arrs else None, len(res_labels),
                                                        res_labels.ctypes.data if res_labels.size else None, videos,
                                                        labels.ctypes.data if labels.size else None, regions,
                                                        (C.c_size_t * max(regions, 1))(*max_items),
                                                        (C.c_uint32 * max(regions, 1))(*min_len), threshold, C.byref(h)))
        self._h = h
        self._grouped = True
        self.lanes, self.max_items, self.min_len, self.threshold = videos * regions, tuple(max_items), tuple(min_len), threshold
        return self

    @property
    def groups(self) -> Optional[np.ndarray]:
        """The labels of all K + N videos, residents first; None for an object without groups."""
        if not getattr(self, "_grouped", False):
            return None
        n = self.resident + self.shape()[0]
        out = np.zeros(max(n, 1), dtype=np.uint32)
        check(lib().needle_hip_crossmatcher_groups(self._h, out.ctypes.data_as(C.POINTER(C.c_uint32)), n))
        return out[:n]

    @staticmethod
    def state_bytes_grouped(groups: Sequence[int], max_items: Sequence[int], resident: Sequence[int] = (),
                            resident_groups: Sequence[int] = ()) -> int:
        """needle_hip_crossmatcher_state_bytes_grouped: `resident` the lengths of the K * regions resident rows in row order;
        0 where creation would refuse."""
        regions = len(max_items)
        seqs = np.zeros((max(len(resident), 1), 2), dtype=np.uint32)
        seqs[:len(resident), 1] = list(resident)
        labels = np.ascontiguousarray(groups, dtype=np.uint32)
        res_labels = np.ascontiguousarray(resident_groups, dtype=np.uint32)
        if len(resident) != len(res_labels) * regions:
            raise ValueError(f"one resident row per video and region: {len(resident)} rows, {len(res_labels)} labels, {regions} regions")
        return int(lib().needle_hip_crossmatcher_state_bytes_grouped(seqs.ctypes.data if len(resident) else None, len(res_labels),
                                                                     res_labels.ctypes.data if res_labels.size else None, labels.size,
                                                                     labels.ctypes.data if labels.size else None, regions,
                                                                     (C.c_size_t * max(regions, 1))(*max_items)))

    @property
    def resident(self) -> int:
        """The known videos the object was created with (0 without `with_resident`)."""
        k = C.c_size_t()
        check(lib().needle_hip_crossmatcher_resident(self._h, C.byref(k)))
        return k.value

    def shape(self) -> Tuple[int, int]:
        """(videos, regions): the arriving videos; the object has videos * regions lanes."""
        videos, regions = C.c_size_t(), C.c_size_t()
        check(lib().needle_hip_crossmatcher_shape(self._h, C.byref(videos), C.byref(regions)))
        return videos.value, regions.value

    @staticmethod
    def state_bytes(lanes: int, max_items, resident: Optional[Sequence[int]] = None) -> int:
        """`max_items`: one capacity, or one per region (`lanes` is then the number of videos).  `resident`: the lengths of the
        K * regions resident rows in row order (`lanes` is then the number of arriving videos)."""
        if resident is not None:
            caps = [max_items] if isinstance(max_items, (int, np.integer)) else list(max_items)
            regions = len(caps)
            if regions and len(resident) % regions:
                raise ValueError(f"one resident row per video and region: {len(resident)} rows, {regions} regions")
            seqs = np.zeros((max(len(resident), 1), 2), dtype=np.uint32)
            seqs[:len(resident), 1] = list(resident)
            return int(lib().needle_hip_crossmatcher_state_bytes_resident(seqs.ctypes.data, len(resident) // max(regions, 1), lanes, regions,
                                                                          (C.c_size_t * max(regions, 1))(*caps)))
        if isinstance(max_items, (int, np.integer)):
            return int(lib().needle_hip_crossmatcher_state_bytes(lanes, max_items))
        regions = len(max_items)
        return int(lib().needle_hip_crossmatcher_state_bytes_regions(lanes, regions, (C.c_size_t * max(regions, 1))(*max_items)))

    def feed(self, items: Sequence) -> None:
        """items[i]: the hashes lane i has received since the last feed, or None / an empty array for nothing."""
        if len(items) != self.lanes:
            raise ValueError(f"one chunk per lane: {self.lanes}, got {len(items)}")
        keep = [None if a is None else np.ascontiguousarray(a, dtype=np.uint32) for a in items]
        ptrs = (C.c_void_p * self.lanes)(*[None if a is None or a.size == 0 else a.ctypes.data for a in keep])
        lens = (C.c_size_t * self.lanes)(*[0 if a is None else a.size for a in keep])
        check(lib().needle_hip_crossmatcher_feed(self._h, ptrs, lens))
        del keep

    def feed_from_feeder(self, feeder: "Feeder") -> None:
        """Takes, lane by lane, the feeder's ready items this matcher has not yet taken; finishes the lanes it has finished."""
        check(lib().needle_hip_crossmatcher_feed_from_feeder(self._h, feeder._h))

    def finish(self, lanes: Optional[Sequence[int]] = None) -> None:
        arr, k = (None, 0) if lanes is None else ((C.c_size_t * max(len(lanes), 1))(*lanes), len(lanes))
        check(lib().needle_hip_crossmatcher_finish(self._h, arr, k))

    def ready(self) -> Tuple[int, bool]:
        """(runs reported, every lane finished)"""
        runs, complete = C.c_size_t(), C.c_bool()
        check(lib().needle_hip_crossmatcher_ready(self._h, C.byref(runs), C.byref(complete)))
        return runs.value, complete.value

    def lane(self, lane: int) -> Tuple[int, bool]:
        """(items fed, finished) of a lane."""
        fed, fin = C.c_uint64(), C.c_bool()
        check(lib().needle_hip_crossmatcher_lane(self._h, lane, C.byref(fed), C.byref(fin)))
        return fed.value, fin.value

    def runs(self, first: int = 0, count: Optional[int] = None) -> np.ndarray:
        if count is None:
            count = self.ready()[0] - first
        out = np.zeros(max(count, 0), dtype=RUN_DTYPE)
        check(lib().needle_hip_crossmatcher_runs(self._h, first, count, out.ctypes.data if count else None))
        return out

    def stats(self) -> Tuple[int, int, int, int]:
        """(feeds, kernel launches, cells evaluated, bytes of state on the device)"""
        out = (C.c_uint64 * 4)()
        check(lib().needle_hip_crossmatcher_stats(self._h, out))
        return tuple(int(x) for x in out)

    def __del__(self):
        if getattr(self, "_h", None):
            lib().needle_hip_crossmatcher_free(self._h)
            self._h = None


def fingerprint(pcms: Sequence[np.ndarray], channels: int = 1, step: int = 1) -> List[np.ndarray]:
    """needle_hip_fingerprint_host: raw chromaprint items (every `step`-th) of each stream."""
    arrs = [np.ascontiguousarray(p, dtype=np.int16) for p in pcms]
    n = len(arrs)
    outs = [np.zeros(max(lib().needle_hip_fingerprint_num_kept(a.size // channels, step), 1), dtype=np.uint32)
            for a in arrs]
    ptrs = (C.c_void_p * max(n, 1))(*[a.ctypes.data for a in arrs])
    lens = (C.c_size_t * max(n, 1))(*[a.size for a in arrs])
    optrs = (C.c_void_p * max(n, 1))(*[o.ctypes.data for o in outs])
    check(lib().needle_hip_fingerprint_host(ptrs, lens, n, channels, step, optrs))
    return [o[:lib().needle_hip_fingerprint_num_kept(a.size // channels, step)] for o, a in zip(outs, arrs)]


def fingerprint_debug(pcm: np.ndarray, channels: int = 1):
    """(chroma [frames][12], features [frames-4][12]) of one stream, computed on the GPU."""
    a = np.ascontiguousarray(pcm, dtype=np.int16)
    samples = a.size // channels
    frames = 0 if samples < 4096 else (samples - 4096) // 1365 + 1
    chroma = np.zeros((max(frames, 1), 12))
    feats = np.zeros((max(frames - 4, 1), 12))
    check(lib().needle_hip_fingerprint_debug(a.ctypes.data, a.size, channels, chroma.ctypes.data, feats.ctypes.data))
    return chroma[:frames], feats[:max(frames - 4, 0)]


class _StageStream(C.Structure):
    _fields_ = [(k, C.c_uint32) for k in ("frames", "frame_base", "pair_base", "kept", "kept_base", "tile_base")]


class _Stages(C.Structure):
    _fields_ = ([(k, C.c_void_p) for k in ("first_chroma", "energy", "first_items", "item_listed", "chunk_listed", "final_chroma",
                                           "items", "streams")] +
                [(k, C.c_uint64) for k in ("frames", "pairs", "kept", "chunks", "items_listed", "chunks_listed")] +
                [(k, C.c_uint32) for k in ("chunk_pairs", "items_per_tile", "compute_units", "pairs_per_block", "pairs_per_xcd",
                                           "blocks_per_xcd")] +
                [("block_size", C.c_uint32 * 4), ("block_count", C.c_uint32 * 4)])


def fingerprint_stages(pcms: Sequence[np.ndarray], channels: int = 1, step: int = 1, beside: bool = False) -> dict:
    """needle_hip_fingerprint_stages_debug (test hook): the product's certified chain over `pcms` as one batch, and what
    each of its kernels wrote.  Rows, pairs, chunks and items are numbered over the batch; `streams` (one dict per stream:
    frames, frame_base, pair_base, kept, kept_base, tile_base) says where each stream's begin.  `schedule` is the first
    pass's: per XCD part of `pairs_per_xcd` pairs, counts[k] workgroups of sizes[k] pairs, in turn."""
    arrs = [np.ascontiguousarray(p, dtype=np.int16) for p in pcms]
    n = len(arrs)
    frames = [0 if a.size // channels < 4096 else (a.size // channels - 4096) // 1365 + 1 for a in arrs]
    kept = [int(lib().needle_hip_fingerprint_num_kept(a.size // channels, step)) for a in arrs]
    nf, nk, pairs = sum(frames), sum(kept), sum((f + 1) // 2 for f in frames)
    out = {"first_chroma": np.zeros((max(nf, 1), 12)), "energy": np.zeros((max(nf, 1), 4), dtype=np.float32),
           "first_items": np.zeros(max(nk, 1), dtype=np.uint32), "item_listed": np.zeros(max(nk, 1), dtype=np.uint8),
           "chunk_listed": np.zeros(max(pairs, 1), dtype=np.uint8), "final_chroma": np.zeros((max(nf, 1), 12)),
           "items": np.zeros(max(nk, 1), dtype=np.uint32)}
    streams = (_StageStream * max(n, 1))()
    st = _Stages(streams=C.addressof(streams), **{k: v.ctypes.data for k, v in out.items()})
    ptrs = (C.c_void_p * max(n, 1))(*[a.ctypes.data for a in arrs])
    lens = (C.c_size_t * max(n, 1))(*[a.size for a in arrs])
    lib().needle_hip_fingerprint_stages_debug.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_uint32, C.c_uint32, C.c_void_p]
    check(lib().needle_hip_fingerprint_stages_debug(ptrs, lens, n, channels, step, 1 if beside else 0, C.byref(st)))
    ran = st.frames > 0
    assert not ran or (st.frames, st.kept, st.pairs) == (nf, nk, pairs), (st.frames, st.kept, st.pairs, nf, nk, pairs)
    rows = {"first_chroma": st.frames, "energy": st.frames, "final_chroma": st.frames, "first_items": st.kept,
            "item_listed": st.kept, "items": st.kept, "chunk_listed": st.chunks}
    res = {k: v[:rows[k]] for k, v in out.items()}
    for k in ("frames", "pairs", "kept", "chunks", "items_listed", "chunks_listed", "chunk_pairs", "items_per_tile", "compute_units",
              "pairs_per_block"):
        res[k] = int(getattr(st, k))
    res["streams"] = [{k: int(getattr(streams[i], k)) for k, _ in _StageStream._fields_} for i in range(n)]
    res["schedule"] = {"pairs_per_xcd": int(st.pairs_per_xcd), "blocks_per_xcd": int(st.blocks_per_xcd),
                       "sizes": [int(x) for x in st.block_size], "counts": [int(x) for x in st.block_count]}
    return res


def resample(pcms: Sequence[np.ndarray], channels: int, sample_rate: int) -> List[np.ndarray]:
    """needle_hip_resample_host: interleaved s16 at `sample_rate` -> mono s16 at 11025 Hz."""
    arrs = [np.ascontiguousarray(p, dtype=np.int16) for p in pcms]
    n = len(arrs)
    lens_out = [lib().needle_hip_resample_out_len(a.size // channels, sample_rate) for a in arrs]
    outs = [np.zeros(max(k, 1), dtype=np.int16) for k in lens_out]
    ptrs = (C.c_void_p * max(n, 1))(*[a.ctypes.data for a in arrs])
    lens = (C.c_size_t * max(n, 1))(*[a.size for a in arrs])
    optrs = (C.c_void_p * max(n, 1))(*[o.ctypes.data for o in outs])
    check(lib().needle_hip_resample_host(ptrs, lens, n, channels, sample_rate, optrs))
    return [o[:k] for o, k in zip(outs, lens_out)]


def resample_plan(sample_rate: int, refused_ok: bool = False) -> dict:
    """needle_hip_resample_plan: which kernel resamples `sample_rate` and its geometry (host arithmetic, no device);
    `family` as its name.  A refused rate raises NeedleError_InvalidArgument unless `refused_ok`."""
    p = CResamplePlan()
    code = lib().needle_hip_resample_plan(int(sample_rate), C.byref(p))
    if code != 0 and not (refused_ok and p.family == RESAMPLE_FAMILIES.index("refused")):
        check(code)
    out = {f: int(getattr(p, f)) for f in RESAMPLE_PLAN_FIELDS}
    out["family"] = RESAMPLE_FAMILIES[out["family"]]
    return out


def resample_plans(lo: int, hi: int) -> np.ndarray:
    """The plans of the rates lo..hi inclusive, as a RESAMPLE_PLAN_DTYPE array (family as its number)."""
    arr = (CResamplePlan * (hi - lo + 1))()
    f = lib().needle_hip_resample_plan
    for i in range(hi - lo + 1):
        f(lo + i, C.byref(arr[i]))
    return np.frombuffer(arr, dtype=RESAMPLE_PLAN_DTYPE).copy()


def downmix(pcms: Sequence[np.ndarray], channels: int) -> List[np.ndarray]:
    """needle_hip_downmix_host: interleaved s16 with `channels` (1..MAX_CHANNELS) channels -> mono s16,
    (sum of a frame) // channels with C truncation toward zero; a trailing partial frame is dropped."""
    arrs = [np.ascontiguousarray(p, dtype=np.int16) for p in pcms]
    n = len(arrs)
    lens_out = [a.size // max(channels, 1) for a in arrs]
    outs = [np.zeros(max(k, 1), dtype=np.int16) for k in lens_out]
    ptrs = (C.c_void_p * max(n, 1))(*[a.ctypes.data for a in arrs])
    lens = (C.c_size_t * max(n, 1))(*[a.size for a in arrs])
    optrs = (C.c_void_p * max(n, 1))(*[o.ctypes.data for o in outs])
    check(lib().needle_hip_downmix_host(ptrs, lens, n, channels, optrs))
    return [o[:k] for o, k in zip(outs, lens_out)]


def convert(pcms: Sequence, channels: int, sample_format: int, num_values: Optional[Sequence[int]] = None) -> List[np.ndarray]:
    """needle_hip_convert_host: streams in `sample_format` (SAMPLE_*; a planar stream is a sequence of `channels` planes)
    -> interleaved `channels`-channel s16, not down-mixed; a trailing partial frame is dropped.  num_values (samples
    over all channels per stream) defaults to the arrays' sizes."""
    keep, flat = _format_pointers(pcms, channels, sample_format)
    n = len(pcms)
    planar = sample_format_planar(sample_format)
    if num_values is None:
        num_values = [sum(q.size for q in p) if planar else np.size(p) for p in pcms]
    lens_out = [int(v) // max(channels, 1) * channels for v in num_values]
    outs = [np.zeros(max(k, 1), dtype=np.int16) for k in lens_out]
    ptrs = (C.c_void_p * max(len(flat), 1))(*flat)
    lens = (C.c_size_t * max(n, 1))(*[int(v) for v in num_values])
    optrs = (C.c_void_p * max(n, 1))(*[o.ctypes.data for o in outs])
    check(lib().needle_hip_convert_host(ptrs, lens, n, channels, sample_format, optrs))
    del keep
    return [o[:k] for o, k in zip(outs, lens_out)]


def convert_mono(pcms: Sequence, formats: Sequence[Tuple[int, int, int]], num_values: Optional[Sequence[int]] = None) -> List[np.ndarray]:
    """needle_hip_convert_mono_host: streams that each have a format of their own -- formats[i] = (channels, sample_rate,
    sample_format), the rate is not looked at -- -> mono s16: `convert`, then `downmix`, in one kernel whatever the mixture.
    num_values (samples over all channels per stream) defaults to the arrays' sizes."""
    formats = [tuple(int(v) for v in f) for f in formats]
    if len(formats) != len(pcms):
        raise ValueError("one format per stream")
    keep, flat, sizes = _lane_pointers(pcms, formats)
    n = len(pcms)
    if num_values is None:
        num_values = sizes
    lens_out = [int(v) // max(f[0], 1) for v, f in zip(num_values, formats)]
    outs = [np.zeros(max(k, 1), dtype=np.int16) for k in lens_out]
    ptrs = (C.c_void_p * max(len(flat), 1))(*flat)
    lens = (C.c_size_t * max(n, 1))(*[int(v) for v in num_values])
    optrs = (C.c_void_p * max(n, 1))(*[o.ctypes.data for o in outs])
    check(lib().needle_hip_convert_mono_host(ptrs, lens, _lane_formats(formats), n, optrs))
    del keep
    return [o[:k] for o, k in zip(outs, lens_out)]


def rematrix_host(pcms: Sequence, formats: Sequence[Tuple[int, int, int]], mixes: Sequence[Optional[ChannelMix]],
                  num_values: Optional[Sequence[int]] = None) -> List[np.ndarray]:
    """needle_hip_rematrix_host: `convert_mono` with a channel mix per stream (None: the plain average of that stream),
    one launch of the rematrix kernel whatever the mixture."""
    formats = [tuple(int(v) for v in f) for f in formats]
    if len(formats) != len(pcms) or len(mixes) != len(pcms):
        raise ValueError("one format and one mix (or None) per stream")
    keep, flat, sizes = _lane_pointers(pcms, formats)
    n = len(pcms)
    if num_values is None:
        num_values = sizes
    lens_out = [int(v) // max(f[0], 1) for v, f in zip(num_values, formats)]
    outs = [np.zeros(max(k, 1), dtype=np.int16) for k in lens_out]
    ptrs = (C.c_void_p * max(len(flat), 1))(*flat)
    lens = (C.c_size_t * max(n, 1))(*[int(v) for v in num_values])
    optrs = (C.c_void_p * max(n, 1))(*[o.ctypes.data for o in outs])
    check(lib().needle_hip_rematrix_host(ptrs, lens, _lane_formats(formats), _channel_mixes(mixes), n, optrs))
    del keep
    return [o[:k] for o, k in zip(outs, lens_out)]


def hamming_runs(seqs: Sequence[np.ndarray], problems: Sequence[Tuple[int, int, int]], threshold: int) -> np.ndarray:
    """needle_hip_hamming_runs_host.  problems: (src_seq, dst_seq, min_len); returns a structured array of
    (problem, src_end, dst_end, len), problem = index into `problems`."""
    arena = np.concatenate([np.ascontiguousarray(s, dtype=np.uint32) for s in seqs]) if seqs else np.zeros(0, np.uint32)
    arena = np.ascontiguousarray(arena, dtype=np.uint32)
    cs = (Seq * max(len(seqs), 1))()
    off = 0
    for i, s in enumerate(seqs):
        cs[i] = Seq(off, len(s))
        off += len(s)
    cp = (Problem * max(len(problems), 1))(*[Problem(a, b, m, i) for i, (a, b, m) in enumerate(problems)])
    runs = C.POINTER(Run)()
    n = C.c_size_t(0)
    check(lib().needle_hip_hamming_runs_host(arena.ctypes.data, arena.size, cs, len(seqs), cp, len(problems),
                                             threshold, C.byref(runs), C.byref(n)))
    out = np.zeros(n.value, dtype=RUN_DTYPE)
    if n.value:
        C.memmove(out.ctypes.data, runs, n.value * C.sizeof(Run))
    lib().needle_hip_host_free(runs)
    return out


# ---- communicator: one process per GPU (include/needle_hip.h, "multi-GPU") --------------------------------------
COMM_ID_BYTES = 128


def comm_create_id() -> bytes:
    buf = (C.c_uint8 * COMM_ID_BYTES)()
    check(lib().needle_hip_comm_create_id(buf))
    return bytes(buf)


def comm_init(comm_id: bytes, rank: int, world: int) -> None:
    assert len(comm_id) == COMM_ID_BYTES
    buf = (C.c_uint8 * COMM_ID_BYTES).from_buffer_copy(comm_id)
    check(lib().needle_hip_comm_init(buf, rank, world))


def comm_finalize() -> None:
    lib().needle_hip_comm_finalize()


def comm_rank() -> int:
    return lib().needle_hip_comm_rank()


def comm_world_size() -> int:
    return lib().needle_hip_comm_world_size()


def comm_backend() -> str:
    return lib().needle_hip_comm_backend().decode()


def comm_barrier() -> None:
    check(lib().needle_hip_comm_barrier())


def comm_all_gather(local: np.ndarray) -> np.ndarray:
    """All-gather of equal-sized host arrays: returns [world, *local.shape]."""
    local = np.ascontiguousarray(local)
    out = np.zeros((comm_world_size(),) + local.shape, dtype=local.dtype)
    check(lib().needle_hip_comm_all_gather_host(local.ctypes.data, out.ctypes.data, local.nbytes))
    return out


def comm_shard(units: int, world: int, rank: int) -> Tuple[int, int]:
    first, count = C.c_size_t(0), C.c_size_t(0)
    lib().needle_hip_comm_shard(units, world, rank, C.byref(first), C.byref(count))
    return first.value, count.value


class CCertAudit(C.Structure):
    _fields_ = [("items", C.c_uint64), ("accepted", C.c_uint64), ("accepted_mismatches", C.c_uint64),
                ("mismatches", C.c_uint64), ("max_error_over_s", C.c_double), ("max_s", C.c_double)]

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _ in self._fields_}


def fingerprint_audit_device(d_pcm: int, pcm_offsets, num_values, channels: int, step: int, d_items: int, item_offsets) -> dict:
    """needle_hip_fingerprint_audit_device: f32 first pass vs f64 kernel over the same resident PCM."""
    n = len(num_values)
    a = CCertAudit()
    u64 = C.c_uint64 * n
    lib().needle_hip_fingerprint_audit_device.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_size_t,
                                                          C.c_int, C.c_uint32, C.c_void_p, C.POINTER(C.c_uint64),
                                                          C.POINTER(CCertAudit)]
    check(lib().needle_hip_fingerprint_audit_device(d_pcm, u64(*pcm_offsets), u64(*num_values), n, channels, step, d_items,
                                                    u64(*item_offsets), C.byref(a)))
    return a.as_dict()


# ---- HBM-resident library (bench / multi-GPU) -----------------------------------------------------------------
class Library:
    """NeedleHipLibrary: PCM resident in HBM, padded device hash arena, pair-sharded search."""

    def __init__(self, num_videos: int, opening_search_percentage: float = DEFAULT_OPENING_SEARCH_PERCENTAGE,
                 hash_duration: float = DEFAULT_HASH_DURATION):
        out = C.c_void_p()
        check(lib().needle_hip_library_new(num_videos, opening_search_percentage, hash_duration, C.byref(out)))
        self._h = out
        self.n = num_videos
        self._format = SAMPLE_S16
        self._formats = None

    def include_endings(self, ending_search_percentage: float = DEFAULT_ENDING_SEARCH_PERCENTAGE) -> "Library":
        check(lib().needle_hip_library_include_endings(self._h, ending_search_percentage))
        return self

    def set_sample_rate(self, sample_rate: int) -> "Library":
        """The rate of the PCM set_pcm / set_pcm_device / stream_pcm / rank_videos will be given; resampled to 11025 Hz
        mono on the device on the way in (needle_hip_library_set_sample_rate)."""
        check(lib().needle_hip_library_set_sample_rate(self._h, sample_rate))
        return self

    def set_groups(self, labels: Sequence[int]) -> "Library":
        """A label per video (0 .. 2^32 - 1, only compared): only pairs inside a group are searched, and pair ids, pair
        ranges and NeedleHipRun.problem are grouped pair ids (needle_hip_library_set_groups; before set_pcm)."""
        k = len(labels)
        arr = (C.c_uint32 * max(k, 1))(*[int(g) for g in labels])
        check(lib().needle_hip_library_set_groups(self._h, arr, k))
        return self

    def groups(self) -> List[int]:
        """The labels of a grouped library, one per video (a plain one: NeedleError)."""
        labels = (C.c_uint32 * max(self.n, 1))()
        check(lib().needle_hip_library_groups(self._h, labels, self.n))
        return list(labels[:self.n])

    def set_channel_mix(self, mix: Optional[ChannelMix]) -> "Library":
        """The PCM of set_pcm / set_pcm_device / stream_pcm is folded to mono with `mix` on the way in
        (needle_hip_library_set_channel_mix; before set_pcm; None: the plain average again)."""
        check(lib().needle_hip_library_set_channel_mix(self._h, None if mix is None else C.byref(mix)))
        return self

    def set_sample_format(self, sample_format: int) -> "Library":
        """The sample format (SAMPLE_*) of the PCM set_pcm / set_pcm_device / stream_pcm will be given; converted to s16
        on the device on the way in (needle_hip_library_set_sample_format).  set_pcm and stream_pcm then pass arrays of
        that format's dtype; a planar video is a sequence of `channels` planes (set_pcm_device: channels pointers per video)."""
        check(lib().needle_hip_library_set_sample_format(self._h, sample_format))
        self._format = sample_format
        return self

    def set_video_formats(self, formats: Sequence[Tuple[int, int, int]],
                          mixes: Optional[Sequence[Optional[ChannelMix]]] = None) -> "Library":
        """A (channels, sample_rate, sample_format) triple per video and, optionally, a mix per video (None: the plain
        average): needle_hip_library_set_video_formats.  set_pcm / set_pcm_device / stream_pcm / rank_videos are then
        called with channels=0; every video gives an array of its format's dtype, a planar one a sequence of its planes
        (set_pcm_device: the concatenation of every video's plane pointers, None for each plane of a video held elsewhere)."""
        if len(formats) != self.n or (mixes is not None and len(mixes) != self.n):
            raise ValueError(f"one format (and one mix) per video is required: {self.n}")
        check(lib().needle_hip_library_set_video_formats(self._h, _lane_formats(formats),
                                                         None if mixes is None else _channel_mixes(mixes)))
        self._formats = [tuple(int(x) for x in f) for f in formats]
        return self

    def video_format(self, video: int) -> Tuple[int, int, int]:
        """(channels, sample_rate, sample_format) of a video (needle_hip_library_video_format)."""
        f = CLaneFormat()
        check(lib().needle_hip_library_video_format(self._h, video, C.byref(f)))
        return f.channels, f.sample_rate, f.format

    def rows_per_video(self) -> int:
        return lib().needle_hip_library_rows_per_video(self._h)

    def _host_pointers(self, pcm, channels: int):
        if self._formats is not None:
            keep, flat, _ = _lane_pointers(pcm, self._formats)
            return keep, (C.c_void_p * max(len(flat), 1))(*flat)
        if self._format == SAMPLE_S16:
            arrs = [None if p is None else np.ascontiguousarray(p, dtype=np.int16) for p in pcm]
            return arrs, (C.c_void_p * self.n)(*[None if a is None else a.ctypes.data for a in arrs])
        keep, flat = _format_pointers(pcm, channels, self._format)
        return keep, (C.c_void_p * max(len(flat), 1))(*flat)

    def set_pcm(self, pcm: Sequence[Optional[np.ndarray]], num_values: Sequence[int], channels: int = 1) -> None:
        arrs, ptrs = self._host_pointers(pcm, channels)
        lens = (C.c_size_t * self.n)(*list(num_values))
        check(lib().needle_hip_library_set_pcm(self._h, ptrs, lens, channels))

    def rank_videos(self, num_values: Sequence[int], world: int, rank: int, channels: int = 1) -> Tuple[int, int]:
        """(first, count) of the videos whose PCM `rank` of `world` must hold (needle_hip_library_rank_videos)."""
        lens = (C.c_size_t * self.n)(*list(num_values))
        first, count = C.c_size_t(0), C.c_size_t(0)
        lib().needle_hip_library_rank_videos.argtypes = [C.c_void_p, C.POINTER(C.c_size_t), C.c_int, C.c_int, C.c_int,
                                                         C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
        check(lib().needle_hip_library_rank_videos(self._h, lens, channels, world, rank, C.byref(first), C.byref(count)))
        return first.value, count.value

    def set_pcm_device(self, d_ptrs: Sequence[Optional[int]], num_values: Sequence[int], channels: int = 1) -> None:
        """PCM already in HBM: device pointers (None for videos of other ranks), copied device to device."""
        ptrs = (C.c_void_p * max(len(d_ptrs), self.n))(*[None if p is None else int(p) for p in d_ptrs])
        lens = (C.c_size_t * self.n)(*list(num_values))
        lib().needle_hip_library_set_pcm_device.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.c_int]
        check(lib().needle_hip_library_set_pcm_device(self._h, ptrs, lens, channels))

    def stream_pcm(self, pcm: Sequence[Optional[np.ndarray]], num_values: Sequence[int], channels: int = 1) -> None:
        """Upload + fingerprint overlapped, PCM not kept (needle_hip_library_stream_pcm)."""
        arrs, ptrs = self._host_pointers(pcm, channels)
        lens = (C.c_size_t * self.n)(*list(num_values))
        check(lib().needle_hip_library_stream_pcm(self._h, ptrs, lens, channels))

    def analyze(self, first: int = 0, count: Optional[int] = None, sync: bool = True) -> None:
        check(lib().needle_hip_library_analyze(self._h, first, self.n - first if count is None else count, sync))

    def hash_arena(self) -> Tuple[int, int]:
        ptr = C.c_void_p()
        stride = C.c_size_t(0)
        check(lib().needle_hip_library_hash_arena(self._h, C.byref(ptr), C.byref(stride)))
        return ptr.value, stride.value

    def use_hash_arena(self, d_ptr: int, rows: int, stride: int) -> None:
        check(lib().needle_hip_library_use_hash_arena(self._h, d_ptr, rows, stride))

    def num_pairs(self) -> int:
        return lib().needle_hip_library_num_pairs(self._h)

    def search(self, comparator: Comparator, first_pair: int, num_pairs: int, d_runs: int, capacity: int,
               d_count: int, sync: bool = True) -> None:
        check(lib().needle_hip_library_search(self._h, comparator._h or comparator.handle(), first_pair, num_pairs,
                                              d_runs, capacity, d_count, sync))

    def fetch_runs_begin(self, slot: int, d_runs: int, d_count: int, max_runs: int) -> None:
        check(lib().needle_hip_library_fetch_runs_begin(self._h, slot, d_runs, d_count, max_runs))

    def fetch_runs_end(self, slot: int, max_runs: int) -> Tuple[np.ndarray, int]:
        """(runs actually downloaded, total found).  The array is a copy, so the slot can be reused."""
        ptr = C.c_void_p()
        total = C.c_uint32(0)
        check(lib().needle_hip_library_fetch_runs_end(self._h, slot, C.byref(ptr), C.byref(total)))
        k = min(total.value, max_runs)
        out = np.zeros(k, dtype=RUN_DTYPE)
        if k:
            C.memmove(out.ctypes.data, ptr.value, k * RUN_DTYPE.itemsize)
        return out, total.value

    def finalize(self, comparator: Comparator, runs: np.ndarray) -> List[Optional[SearchResult]]:
        runs = np.ascontiguousarray(runs, dtype=RUN_DTYPE)
        res = (CSearchResult * self.n)()
        check(lib().needle_hip_library_finalize(self._h, comparator._h or comparator.handle(), runs.ctypes.data,
                                                runs.size, res))
        return _results(res, self.n)

    def frame_hashes(self, index: int) -> FrameHashes:
        out = C.c_void_p()
        check(lib().needle_hip_library_frame_hashes(self._h, index, C.byref(out)))
        return FrameHashes(out.value, True)

    def job_begin(self, comparator: Comparator, slot: int = 0) -> None:
        """Enqueues one analyze+search job of this rank's share (all of it without a communicator)."""
        check(lib().needle_hip_library_job_begin(self._h, comparator._h or comparator.handle(), slot))

    def job_end(self, comparator: Comparator, slot: int = 0) -> Tuple[List[Optional[SearchResult]], int]:
        """(results for all videos -- the same on every rank, runs found over all pairs)."""
        res = (CSearchResult * self.n)()
        found = C.c_size_t(0)
        check(lib().needle_hip_library_job_end(self._h, comparator._h or comparator.handle(), slot, res, C.byref(found)))
        return _results(res, self.n), found.value

    def audit(self) -> dict:
        """Both transforms over this rank's resident PCM, every kept item compared on the device (needle_hip_library_audit)."""
        a = CCertAudit()
        lib().needle_hip_library_audit.argtypes = [C.c_void_p, C.POINTER(CCertAudit)]
        check(lib().needle_hip_library_audit(self._h, C.byref(a)))
        return a.as_dict()

    def job_runs(self, slot: int = 0) -> np.ndarray:
        """The complete run list of the job that finished last in `slot` (a copy; needle_hip_library_job_runs)."""
        ptr, total = C.c_void_p(), C.c_size_t(0)
        lib().needle_hip_library_job_runs.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
        check(lib().needle_hip_library_job_runs(self._h, slot, C.byref(ptr), C.byref(total)))
        out = np.zeros(total.value, dtype=RUN_DTYPE)
        if total.value:
            C.memmove(out.ctypes.data, ptr.value, out.nbytes)
        return out

    def job_form(self, slot: int = 0) -> dict:
        """Which forms the slot's last finished job took (needle_hip_library_job_form)."""
        f = (C.c_uint32 * 4)()
        lib().needle_hip_library_job_form.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_uint32)]
        check(lib().needle_hip_library_job_form(self._h, slot, f))
        return {"device_epilogue": bool(f[0]), "sharded_epilogue": bool(f[1]), "directed_runs": bool(f[2]), "scan_form": int(f[3])}

    def job_comm_bytes(self, slot: int = 0) -> dict:
        b = (C.c_uint64 * 4)()
        lib().needle_hip_library_job_comm_bytes.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_uint64)]
        check(lib().needle_hip_library_job_comm_bytes(self._h, slot, b))
        return {"hash_rows": int(b[0]), "run_heads": int(b[1]), "results": int(b[2]), "scans_repeated": int(b[3])}

    def __del__(self):
        if getattr(self, "_h", None):
            lib().needle_hip_library_free(self._h)
            self._h = None


class PinnedArray:
    """An int16 numpy array over page-locked host memory (needle_hip_host_alloc): PCM the copy engine reads in place."""

    def __init__(self, count: int):
        p = C.c_void_p()
        check(lib().needle_hip_host_alloc(C.byref(p), max(count, 1) * 2))
        self.ptr = p.value
        self.array = np.ctypeslib.as_array((C.c_int16 * max(count, 1)).from_address(self.ptr))[:count]

    def __del__(self):
        if getattr(self, "ptr", None):
            self.array = None
            lib().needle_hip_host_alloc_free(self.ptr)
            self.ptr = None


class DeviceBuffer:
    """hipMalloc'd scratch owned by Python (run lists, counters)."""

    def __init__(self, nbytes: int):
        p = C.c_void_p()
        check(lib().needle_hip_malloc(C.byref(p), nbytes))
        self.ptr = p.value
        self.nbytes = nbytes

    def to_host(self, dtype, count: int) -> np.ndarray:
        out = np.zeros(count, dtype=dtype)
        if count:
            check(lib().needle_hip_memcpy_d2h(out.ctypes.data, self.ptr, out.nbytes))
        return out

    def __del__(self):
        if getattr(self, "ptr", None):
            lib().needle_hip_free(self.ptr)
            self.ptr = None
