//! Raw declarations of include/needle.h and the part of include/needle_hip.h this crate uses.
//! Keep in step with those headers; tests/test_capi_cpu.py checks that the library exports every symbol.
#![allow(non_camel_case_types, dead_code)]

use std::os::raw::{c_char, c_int, c_void};

/// `enum NeedleError` (needle-capi/src/lib.rs:58-85): repr(C), values 0..=11.
#[repr(C)]
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub enum NeedleError {
    Ok = 0,
    InvalidUtf8String,
    NullArgument,
    InvalidArgument,
    FrameHashDataNotFound,
    FrameHashDataInvalidVersion,
    InvalidFrameHashData,
    ComparatorMinimumPaths,
    AnalyzerInvalidHashPeriod,
    AnalyzerInvalidHashDuration,
    IOError,
    Unknown,
}

#[repr(C)]
pub struct NeedleAudioAnalyzer {
    _private: [u8; 0],
}
#[repr(C)]
pub struct NeedleAudioComparator {
    _private: [u8; 0],
}
#[repr(C)]
pub struct FrameHashes {
    _private: [u8; 0],
}

#[repr(C)]
pub struct NeedleHipLibrary {
    _private: [u8; 0],
}

#[repr(C)]
pub struct NeedleHipFeeder {
    _private: [u8; 0],
}
#[repr(C)]
pub struct NeedleHipMatcher {
    _private: [u8; 0],
}
#[repr(C)]
pub struct NeedleHipCrossMatcher {
    _private: [u8; 0],
}
#[repr(C)]
pub struct NeedleHipIndex {
    _private: [u8; 0],
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct NeedleHipSearchResult {
    pub has_result: bool,
    pub has_opening: bool,
    pub has_ending: bool,
    pub opening_start_ns: u64,
    pub opening_end_ns: u64,
    pub ending_start_ns: u64,
    pub ending_end_ns: u64,
}

/// Why a region of a video got its match (`NeedleHipMatchEvidence`, include/needle_hip.h): the winner of
/// `find_best_match`, its pair and the candidates that agree with it.  `partner == u32::MAX`: no match, every other field 0.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq)]
pub struct NeedleHipMatchEvidence {
    pub partner: u32,
    pub is_source: u32,
    pub candidate: u32,
    pub candidates: u32,
    pub support: u32,
    pub partners: u32,
    pub score: f32,
    pub match_hash: u32,
    pub partner_hash: u32,
    pub reserved: u32,
    pub start_ns: u64,
    pub end_ns: u64,
    pub partner_start_ns: u64,
    pub partner_end_ns: u64,
}

/// `NeedleHipSearchEvidence`: the opening's record and the ending's.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq)]
pub struct NeedleHipSearchEvidence {
    pub(crate) opening: NeedleHipMatchEvidence,
    pub(crate) ending: NeedleHipMatchEvidence,
}

impl NeedleHipSearchEvidence {
    pub fn opening(&self) -> NeedleHipMatchEvidence {
        self.opening
    }
    pub fn ending(&self) -> NeedleHipMatchEvidence {
        self.ending
    }
}

/// One sequence inside a hash arena (`NeedleHipSeq`, include/needle_hip.h).
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct NeedleHipSeq {
    pub offset: u32,
    pub len: u32,
}

/// One matched segment of a pair (`NeedleHipRun`, include/needle_hip.h): what
/// `Comparator::longest_common_hash_match` pushes per maximal run (comparator.rs:196-229).
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct NeedleHipRun {
    pub problem: u32,
    pub src_end: u32,
    pub dst_end: u32,
    pub len: u32,
    pub src_match_hash: u32,
    pub dst_match_hash: u32,
}

/// Result of `needle_hip_library_audit` (f32 first pass vs the f64 kernel over the same resident PCM).
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct NeedleHipCertAudit {
    pub items: u64,
    pub accepted: u64,
    pub accepted_mismatches: u64,
    pub mismatches: u64,
    pub max_error_over_s: f64,
    pub max_s: f64,
}

/// A feeder lane's (or a stream's) channel count, sample rate and `NeedleHipSampleFormat`.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct NeedleHipLaneFormat {
    pub channels: i32,
    pub sample_rate: i32,
    pub format: i32,
}

/// One segment of a feeder lane's stream (`needle_hip_feeder_switch_format`): its format and the frames fed in it.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct NeedleHipSegment {
    pub(crate) format: NeedleHipLaneFormat,
    pub(crate) frames: u64,
}

impl NeedleHipSegment {
    pub fn new(format: NeedleHipLaneFormat, frames: u64) -> Self {
        Self { format, frames }
    }
    pub fn format(&self) -> NeedleHipLaneFormat {
        self.format
    }
    /// Samples per channel fed in that format.
    pub fn frames(&self) -> u64 {
        self.frames
    }
}

/// A channel mix: a 2 x C matrix of Q15 integers, `coef[0][c]` to the left output and `coef[1][c]` to the right
/// (`needle_hip.h`, "Channel mixes").  `channels == 0` stands for "no mix" where an array of mixes is passed.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct NeedleHipChannelMix {
    pub(crate) channels: i32,
    pub(crate) coef: [[i32; 8]; 2],
}

impl NeedleHipChannelMix {
    /// The mix of `left.len()` channels with these two rows (at most 8 coefficients each).
    pub fn new(left: &[i32], right: &[i32]) -> Self {
        assert!(left.len() == right.len() && left.len() <= 8, "two rows of at most 8 coefficients each");
        let mut m = Self { channels: left.len() as i32, coef: [[0; 8]; 2] };
        m.coef[0][..left.len()].copy_from_slice(left);
        m.coef[1][..right.len()].copy_from_slice(right);
        m
    }
    pub fn channels(&self) -> i32 {
        self.channels
    }
    /// The left (0) or right (1) row, `channels` coefficients.
    pub fn row(&self, output: usize) -> &[i32] {
        &self.coef[output][..self.channels.clamp(0, 8) as usize]
    }
}

extern "C" {
    // ---- needle.h ------------------------------------------------------------------------------------
    pub fn needle_error_to_str(error: NeedleError) -> *const c_char;
    pub fn needle_audio_analyzer_new(
        paths: *const *const c_char,
        num_paths: usize,
        opening_search_percentage: f32,
        ending_search_percentage: f32,
        include_endings: bool,
        threaded_decoding: bool,
        force: bool,
        output: *mut *mut NeedleAudioAnalyzer,
    ) -> NeedleError;
    pub fn needle_audio_analyzer_free(analyzer: *const NeedleAudioAnalyzer);
    pub fn needle_audio_analyzer_get_frame_hashes(
        analyzer: *const NeedleAudioAnalyzer,
        index: usize,
        output: *mut *const FrameHashes,
    ) -> NeedleError;
    pub fn needle_audio_analyzer_run(
        analyzer: *mut NeedleAudioAnalyzer,
        hash_duration: f32,
        persist: bool,
        threading: bool,
    ) -> NeedleError;
    pub fn needle_audio_comparator_new(
        paths: *const *const c_char,
        num_paths: usize,
        include_endings: bool,
        hash_match_threshold: u16,
        min_opening_duration: u16,
        min_ending_duration: u16,
        time_padding: f32,
        output: *mut *const NeedleAudioComparator,
    ) -> NeedleError;
    pub fn needle_audio_comparator_free(comparator: *const NeedleAudioComparator);
    pub fn needle_audio_comparator_run(
        comparator: *const NeedleAudioComparator,
        analyze: bool,
        display: bool,
        use_skip_files: bool,
        write_skip_files: bool,
        threading: bool,
    ) -> NeedleError;

    // ---- needle_hip.h --------------------------------------------------------------------------------
    pub fn needle_hip_last_error_message() -> *const c_char;
    pub fn needle_hip_device_count(count: *mut c_int) -> NeedleError;
    pub fn needle_hip_set_device(ordinal: c_int) -> NeedleError;
    pub fn needle_hip_synchronize() -> NeedleError;
    /// PCI address of the current device ("0000:c1:00.0", NUL-terminated) into a 32-byte buffer.
    pub fn needle_hip_device_pci_bus_id(out: *mut c_char) -> NeedleError;
    /// {items, items recomputed in f64, chunks, chunks recomputed} of the certified f32 first pass.
    pub fn needle_hip_fingerprint_cert_stats(counts: *mut u64, reset: bool) -> NeedleError;
    /// Cell evaluations issued by the counting instantiation of the scan (NEEDLE_HIP_SCAN_COUNT=1).
    pub fn needle_hip_scan_issued_evaluations(lane_evaluations: *mut u64, reset: bool) -> NeedleError;
    /// Form of this process's last scan launch (3: aligned windows on the vector ALU, 4: head rows on the matrix pipe)
    /// and, for form 4, the matrix instructions it issued.
    pub fn needle_hip_scan_last_launch(form: *mut i32, matrix_products: *mut u64) -> NeedleError;
    pub fn needle_hip_epilogue_host_fallbacks(jobs: *mut u64, reset: bool) -> NeedleError;
    /// The library's `hipStream_t` on the current device (NULL without one).
    pub fn needle_hip_stream() -> *mut c_void;
    pub fn needle_hip_analyzer_run_pcm(
        analyzer: *mut NeedleAudioAnalyzer,
        pcm: *const *const i16,
        num_values: *const usize,
        channels: c_int,
        sample_rate: c_int,
        hash_duration: f32,
        persist: bool,
    ) -> NeedleError;
    /// `needle_hip_analyzer_run_pcm` with the samples in `format` (`NeedleHipSampleFormat`, FFmpeg's `AVSampleFormat`
    /// numbering: 0-4 u8 / s16 / s32 / f32 / f64 interleaved, 5-9 the same planar with videos x channels pointers),
    /// converted to s16 on the device.
    pub fn needle_hip_analyzer_run_pcm_format(
        analyzer: *mut NeedleAudioAnalyzer,
        pcm: *const *const c_void,
        num_values: *const usize,
        channels: c_int,
        sample_rate: c_int,
        format: c_int,
        hash_duration: f32,
        persist: bool,
    ) -> NeedleError;
    pub fn needle_hip_comparator_run_with_frame_hashes(
        comparator: *const NeedleAudioComparator,
        frame_hashes: *const *const FrameHashes,
        num_videos: usize,
        display: bool,
        use_skip_files: bool,
        write_skip_files: bool,
        results: *mut NeedleHipSearchResult,
    ) -> NeedleError;
    pub fn needle_hip_frame_hashes_new(
        opening_hashes: *const u32,
        opening_ts_ns: *const u64,
        num_opening: usize,
        ending_hashes: *const u32,
        ending_ts_ns: *const u64,
        num_ending: usize,
        hash_duration_ns: u64,
        md5: *const c_char,
        output: *mut *mut FrameHashes,
    ) -> NeedleError;
    pub fn needle_hip_frame_hashes_free(frame_hashes: *mut FrameHashes);
    pub fn needle_hip_frame_hashes_len(frame_hashes: *const FrameHashes, ending: bool) -> usize;
    pub fn needle_hip_frame_hashes_copy(
        frame_hashes: *const FrameHashes,
        ending: bool,
        hashes: *mut u32,
        ts_ns: *mut u64,
        capacity: usize,
    ) -> NeedleError;
    pub fn needle_hip_frame_hashes_hash_duration_ns(frame_hashes: *const FrameHashes) -> u64;
    pub fn needle_hip_frame_hashes_md5(frame_hashes: *const FrameHashes) -> *const c_char;
    pub fn needle_hip_frame_hashes_read(path: *const c_char, output: *mut *mut FrameHashes) -> NeedleError;
    pub fn needle_hip_frame_hashes_write(frame_hashes: *const FrameHashes, path: *const c_char) -> NeedleError;
    // ---- multi-GPU: one process per GPU, RCCL inside the library (include/needle_hip.h "multi-GPU") ----
    pub fn needle_hip_comm_create_id(id: *mut u8) -> NeedleError; // NEEDLE_HIP_COMM_ID_BYTES = 128
    pub fn needle_hip_comm_init(id: *const u8, rank: c_int, world_size: c_int) -> NeedleError;
    pub fn needle_hip_comm_finalize();
    pub fn needle_hip_comm_rank() -> c_int;
    pub fn needle_hip_comm_world_size() -> c_int;
    pub fn needle_hip_comm_barrier() -> NeedleError;
    pub fn needle_hip_comm_all_gather_host(send: *const c_void, recv: *mut c_void, bytes_per_rank: usize) -> NeedleError;
    pub fn needle_hip_comm_shard(units: usize, world_size: c_int, rank: c_int, first: *mut usize, count: *mut usize);
    pub fn needle_hip_library_new(
        num_videos: usize,
        opening_search_percentage: f32,
        hash_duration: f32,
        output: *mut *mut NeedleHipLibrary,
    ) -> NeedleError;
    pub fn needle_hip_library_free(library: *mut NeedleHipLibrary);
    // ---- incremental index (include/needle_hip.h "Incremental index") ----
    pub fn needle_hip_index_new(comparator: *const NeedleAudioComparator, output: *mut *mut NeedleHipIndex) -> NeedleError;
    pub fn needle_hip_index_free(index: *mut NeedleHipIndex);
    pub fn needle_hip_index_len(index: *const NeedleHipIndex) -> usize;
    pub fn needle_hip_index_add(index: *mut NeedleHipIndex, frame_hashes: *const *const FrameHashes, k: usize) -> NeedleError;
    pub fn needle_hip_index_results(index: *const NeedleHipIndex, results: *mut NeedleHipSearchResult, n: usize) -> NeedleError;
    pub fn needle_hip_index_evidence(index: *const NeedleHipIndex, evidence: *mut NeedleHipSearchEvidence, n: usize) -> NeedleError;
    pub fn needle_hip_comparator_results_from_runs_evidence(
        comparator: *const NeedleAudioComparator,
        frame_hashes: *const *const FrameHashes,
        num_videos: usize,
        runs: *const NeedleHipRun,
        num_runs: usize,
        first_video: usize,
        video_count: usize,
        results: *mut NeedleHipSearchResult,
        evidence: *mut NeedleHipSearchEvidence,
    ) -> NeedleError;
    // ---- groups of videos (include/needle_hip.h "A library of many shows") ----
    pub fn needle_hip_group_pairs(
        groups: *const u32,
        num_videos: usize,
        pair_videos: *mut u32,
        capacity: usize,
        num_pairs: *mut u64,
    ) -> NeedleError;
    pub fn needle_hip_comparator_run_with_frame_hashes_grouped(
        comparator: *const NeedleAudioComparator,
        frame_hashes: *const *const FrameHashes,
        num_videos: usize,
        groups: *const u32,
        display: bool,
        use_skip_files: bool,
        write_skip_files: bool,
        results: *mut NeedleHipSearchResult,
    ) -> NeedleError;
    pub fn needle_hip_comparator_results_from_runs_grouped(
        comparator: *const NeedleAudioComparator,
        frame_hashes: *const *const FrameHashes,
        num_videos: usize,
        groups: *const u32,
        runs: *const NeedleHipRun,
        num_runs: usize,
        results: *mut NeedleHipSearchResult,
    ) -> NeedleError;
    pub fn needle_hip_comparator_run_grouped(
        comparator: *const NeedleAudioComparator,
        groups: *const u32,
        num_groups_entries: usize,
        analyze: bool,
        display: bool,
        use_skip_files: bool,
        write_skip_files: bool,
    ) -> NeedleError;
    pub fn needle_hip_index_pairs_searched(index: *const NeedleHipIndex, total: *mut u64, last: *mut u64) -> NeedleError;
    pub fn needle_hip_index_remove(index: *mut NeedleHipIndex, positions: *const usize, k: usize) -> NeedleError;
    pub fn needle_hip_index_replace(
        index: *mut NeedleHipIndex,
        positions: *const usize,
        frame_hashes: *const *const FrameHashes,
        k: usize,
    ) -> NeedleError;
    pub fn needle_hip_index_store_sizes(index: *const NeedleHipIndex, sizes: *mut u64) -> NeedleError;
    pub fn needle_hip_index_crossmatcher_new(
        index: *mut NeedleHipIndex,
        videos: usize,
        max_items: *const usize,
        min_len: *const u32,
        output: *mut *mut NeedleHipCrossMatcher,
    ) -> NeedleError;
    pub fn needle_hip_index_add_matched(
        index: *mut NeedleHipIndex,
        matcher: *mut NeedleHipCrossMatcher,
        frame_hashes: *const *const FrameHashes,
        k: usize,
    ) -> NeedleError;
    pub fn needle_hip_index_crossmatcher_new_grouped(
        index: *mut NeedleHipIndex,
        videos: usize,
        groups: *const u32,
        max_items: *const usize,
        min_len: *const u32,
        output: *mut *mut NeedleHipCrossMatcher,
    ) -> NeedleError;
    pub fn needle_hip_index_add_matched_grouped(
        index: *mut NeedleHipIndex,
        matcher: *mut NeedleHipCrossMatcher,
        frame_hashes: *const *const FrameHashes,
        k: usize,
    ) -> NeedleError;
    pub fn needle_hip_index_matcher_new(index: *mut NeedleHipIndex, videos: usize, output: *mut *mut NeedleHipMatcher) -> NeedleError;
    pub fn needle_hip_index_add_streamed(
        index: *mut NeedleHipIndex,
        matcher: *mut NeedleHipMatcher,
        crossmatcher: *mut NeedleHipCrossMatcher,
        frame_hashes: *const *const FrameHashes,
        k: usize,
    ) -> NeedleError;
    pub fn needle_hip_index_pairs_scanned(index: *const NeedleHipIndex, total: *mut u64, last: *mut u64) -> NeedleError;
    pub fn needle_hip_index_new_grouped(comparator: *const NeedleAudioComparator, output: *mut *mut NeedleHipIndex) -> NeedleError;
    pub fn needle_hip_index_add_grouped(
        index: *mut NeedleHipIndex,
        frame_hashes: *const *const FrameHashes,
        groups: *const u32,
        k: usize,
    ) -> NeedleError;
    pub fn needle_hip_index_groups(index: *const NeedleHipIndex, labels: *mut u32, n: usize) -> NeedleError;
    /// 1..=MAX_CHANNELS interleaved channels -> mono, `(sum of a frame) / channels` with C truncation; `out[i]` holds
    /// `num_values[i] / channels` values.
    pub fn needle_hip_downmix_host(
        pcm: *const *const i16,
        num_values: *const usize,
        num_streams: usize,
        channels: c_int,
        out: *const *mut i16,
    ) -> NeedleError;
    /// The conversion on its own: `out[i]` receives interleaved `channels`-channel s16 (`num_values[i] / channels * channels`
    /// values), not down-mixed.
    pub fn needle_hip_convert_host(
        pcm: *const *const c_void,
        num_values: *const usize,
        num_streams: usize,
        channels: c_int,
        format: c_int,
        out: *const *mut i16,
    ) -> NeedleError;
    /// The sample format of the PCM `set_pcm`, `set_pcm_device` and `stream_pcm` will be given (callers cast their pointers).
    pub fn needle_hip_library_set_sample_format(library: *mut NeedleHipLibrary, format: c_int) -> NeedleError;
    pub fn needle_hip_library_include_endings(library: *mut NeedleHipLibrary, ending_search_percentage: f32) -> NeedleError;
    pub fn needle_hip_library_set_sample_rate(library: *mut NeedleHipLibrary, sample_rate: c_int) -> NeedleError;
    pub fn needle_hip_library_set_groups(library: *mut NeedleHipLibrary, groups: *const u32, num_videos: usize) -> NeedleError;
    pub fn needle_hip_library_groups(library: *const NeedleHipLibrary, labels: *mut u32, n: usize) -> NeedleError;
    pub fn needle_hip_library_set_pcm(
        library: *mut NeedleHipLibrary,
        pcm: *const *const i16,
        num_values: *const usize,
        channels: c_int,
    ) -> NeedleError;
    /// Videos `[first_video, first_video + video_count)` whose PCM rank `rank` of `world_size` must hold.
    pub fn needle_hip_library_rank_videos(
        library: *const NeedleHipLibrary,
        num_values: *const usize,
        channels: c_int,
        world_size: c_int,
        rank: c_int,
        first_video: *mut usize,
        video_count: *mut usize,
    ) -> NeedleError;
    /// `d_pcm[i]` are DEVICE pointers (PCM decoded or generated on the GPU), NULL for videos of other ranks.
    pub fn needle_hip_library_set_pcm_device(
        library: *mut NeedleHipLibrary,
        d_pcm: *const *const i16,
        num_values: *const usize,
        channels: c_int,
    ) -> NeedleError;
    pub fn needle_hip_library_stream_pcm(
        library: *mut NeedleHipLibrary,
        pcm: *const *const i16,
        num_values: *const usize,
        channels: c_int,
    ) -> NeedleError;
    pub fn needle_hip_library_job_begin(
        library: *mut NeedleHipLibrary,
        comparator: *const NeedleAudioComparator,
        slot: c_int,
    ) -> NeedleError;
    pub fn needle_hip_library_job_end(
        library: *mut NeedleHipLibrary,
        comparator: *const NeedleAudioComparator,
        slot: c_int,
        results: *mut NeedleHipSearchResult,
        num_runs: *mut usize,
    ) -> NeedleError;
    pub fn needle_hip_library_frame_hashes(
        library: *mut NeedleHipLibrary,
        index: usize,
        output: *mut *mut FrameHashes,
    ) -> NeedleError;
    /// The complete run list of the job that finished last in `slot`; valid until the slot's next `job_begin`.
    pub fn needle_hip_library_job_runs(
        library: *const NeedleHipLibrary,
        slot: c_int,
        runs: *mut *const NeedleHipRun,
        num_runs: *mut usize,
    ) -> NeedleError;
    /// `{hash rows, run heads, results}` bytes received in the job's all-gathers, `[3]` = scans repeated.
    pub fn needle_hip_library_job_comm_bytes(library: *const NeedleHipLibrary, slot: c_int, bytes: *mut u64) -> NeedleError;
    pub fn needle_hip_library_job_form(library: *const NeedleHipLibrary, slot: c_int, form: *mut u32) -> NeedleError;
    pub fn needle_hip_library_audit(library: *mut NeedleHipLibrary, audit: *mut NeedleHipCertAudit) -> NeedleError;
    pub fn needle_hip_host_threads() -> c_int;
    pub fn needle_hip_host_alloc(host_ptr: *mut *mut c_void, bytes: usize) -> NeedleError;
    pub fn needle_hip_host_alloc_free(host_ptr: *mut c_void) -> NeedleError;
    /// Streaming fingerprinter: chromaprint's start / feed / finish batched over lanes, state on the device.
    pub fn needle_hip_feeder_new(
        lanes: usize,
        channels: c_int,
        sample_rate: c_int,
        format: c_int,
        step: u32,
        output: *mut *mut NeedleHipFeeder,
    ) -> NeedleError;
    pub fn needle_hip_feeder_new_lanes(formats: *const NeedleHipLaneFormat, lanes: usize, step: u32, output: *mut *mut NeedleHipFeeder) -> NeedleError;
    pub fn needle_hip_feeder_lane_format(feeder: *const NeedleHipFeeder, lane: usize, format: *mut NeedleHipLaneFormat) -> NeedleError;
    pub fn needle_hip_feeder_reset_format(
        feeder: *mut NeedleHipFeeder,
        lanes: *const usize,
        formats: *const NeedleHipLaneFormat,
        k: usize,
    ) -> NeedleError;
    pub fn needle_hip_convert_mono_host(
        pcm: *const *const c_void,
        num_values: *const usize,
        formats: *const NeedleHipLaneFormat,
        num_streams: usize,
        out: *const *mut i16,
    ) -> NeedleError;
    pub fn needle_hip_channel_mix_default(channel_mask: u32, out: *mut NeedleHipChannelMix) -> NeedleError;
    pub fn needle_hip_rematrix_host(
        pcm: *const *const c_void,
        num_values: *const usize,
        formats: *const NeedleHipLaneFormat,
        mixes: *const NeedleHipChannelMix,
        num_streams: usize,
        out: *const *mut i16,
    ) -> NeedleError;
    pub fn needle_hip_analyzer_set_channel_mix(analyzer: *mut NeedleAudioAnalyzer, mix: *const NeedleHipChannelMix) -> NeedleError;
    pub fn needle_hip_analyzer_set_layout_downmix(analyzer: *mut NeedleAudioAnalyzer, on: bool) -> NeedleError;
    pub fn needle_hip_comparator_set_layout_downmix(comparator: *mut NeedleAudioComparator, on: bool) -> NeedleError;
    pub fn needle_hip_library_set_channel_mix(library: *mut NeedleHipLibrary, mix: *const NeedleHipChannelMix) -> NeedleError;
    pub fn needle_hip_library_set_video_formats(
        library: *mut NeedleHipLibrary,
        formats: *const NeedleHipLaneFormat,
        mixes: *const NeedleHipChannelMix,
    ) -> NeedleError;
    pub fn needle_hip_library_video_format(library: *const NeedleHipLibrary, video: usize, format: *mut NeedleHipLaneFormat) -> NeedleError;
    pub fn needle_hip_analyzer_run_pcm_formats(
        analyzer: *mut NeedleAudioAnalyzer,
        pcm: *const *const c_void,
        num_values: *const usize,
        formats: *const NeedleHipLaneFormat,
        mixes: *const NeedleHipChannelMix,
        hash_duration: f32,
        persist: bool,
    ) -> NeedleError;
    pub fn needle_hip_feeder_set_lane_mix(
        feeder: *mut NeedleHipFeeder,
        lanes: *const usize,
        mixes: *const NeedleHipChannelMix,
        k: usize,
    ) -> NeedleError;
    pub fn needle_hip_feeder_switch_format(
        feeder: *mut NeedleHipFeeder,
        lanes: *const usize,
        formats: *const NeedleHipLaneFormat,
        mixes: *const NeedleHipChannelMix,
        k: usize,
    ) -> NeedleError;
    pub fn needle_hip_feeder_lane_segments(
        feeder: *const NeedleHipFeeder,
        lane: usize,
        out: *mut NeedleHipSegment,
        cap: usize,
        count: *mut usize,
    ) -> NeedleError;
    pub fn needle_hip_feeder_num_ready_segments(segments: *const NeedleHipSegment, count: usize, step: u32, finished: bool) -> usize;
    pub fn needle_hip_feeder_free(feeder: *mut NeedleHipFeeder);
    pub fn needle_hip_feeder_feed(feeder: *mut NeedleHipFeeder, pcm: *const *const c_void, num_values: *const usize) -> NeedleError;
    pub fn needle_hip_feeder_finish(feeder: *mut NeedleHipFeeder, lanes: *const usize, k: usize) -> NeedleError;
    pub fn needle_hip_feeder_reset(feeder: *mut NeedleHipFeeder, lanes: *const usize, k: usize) -> NeedleError;
    pub fn needle_hip_feeder_ready(
        feeder: *mut NeedleHipFeeder,
        lane: usize,
        kept_items: *mut usize,
        samples_per_channel_fed: *mut u64,
        finished: *mut bool,
    ) -> NeedleError;
    pub fn needle_hip_feeder_items(feeder: *mut NeedleHipFeeder, lane: usize, first: usize, count: usize, items: *mut u32) -> NeedleError;
    pub fn needle_hip_feeder_frame_hashes(
        feeder: *mut NeedleHipFeeder,
        opening_lane: usize,
        ending_lane: usize,
        ending_seek_ns: u64,
        hash_duration: f32,
        md5: *const c_char,
        output: *mut *mut FrameHashes,
    ) -> NeedleError;
    pub fn needle_hip_feeder_state_bytes(feeder: *const NeedleHipFeeder, bytes: *mut u64) -> NeedleError;
    pub fn needle_hip_feeder_set_audit(feeder: *mut NeedleHipFeeder, on: bool) -> NeedleError;
    pub fn needle_hip_feeder_audit(feeder: *mut NeedleHipFeeder, lane: usize, audit: *mut NeedleHipCertAudit) -> NeedleError;
    pub fn needle_hip_feeder_num_ready(
        samples_per_channel_fed: u64,
        sample_rate: c_int,
        channels: c_int,
        step: u32,
        finished: bool,
    ) -> usize;
    /// Streaming comparator: resident sources against lanes of hashes that arrive in chunks, run lengths on the device.
    pub fn needle_hip_matcher_new(
        hashes: *const u32,
        num_hashes: usize,
        sources: *const NeedleHipSeq,
        min_len: *const u32,
        num_sources: usize,
        lanes: usize,
        threshold: u32,
        output: *mut *mut NeedleHipMatcher,
    ) -> NeedleError;
    pub fn needle_hip_matcher_new_regions(
        hashes: *const u32,
        num_hashes: usize,
        sources: *const NeedleHipSeq,
        min_len: *const u32,
        num_sources: usize,
        regions: usize,
        lanes: usize,
        threshold: u32,
        output: *mut *mut NeedleHipMatcher,
    ) -> NeedleError;
    pub fn needle_hip_matcher_free(matcher: *mut NeedleHipMatcher);
    pub fn needle_hip_matcher_feed(matcher: *mut NeedleHipMatcher, items: *const *const u32, num_items: *const usize) -> NeedleError;
    pub fn needle_hip_matcher_feed_from_feeder(matcher: *mut NeedleHipMatcher, feeder: *mut NeedleHipFeeder) -> NeedleError;
    pub fn needle_hip_matcher_finish(matcher: *mut NeedleHipMatcher, lanes: *const usize, k: usize) -> NeedleError;
    pub fn needle_hip_matcher_reset(matcher: *mut NeedleHipMatcher, lanes: *const usize, k: usize) -> NeedleError;
    pub fn needle_hip_matcher_ready(
        matcher: *mut NeedleHipMatcher,
        lane: usize,
        num_runs: *mut usize,
        items_fed: *mut u64,
        finished: *mut bool,
    ) -> NeedleError;
    pub fn needle_hip_matcher_runs(matcher: *mut NeedleHipMatcher, lane: usize, first: usize, count: usize, runs: *mut NeedleHipRun) -> NeedleError;
    pub fn needle_hip_matcher_open(matcher: *mut NeedleHipMatcher, lane: usize, runs: *mut *mut NeedleHipRun, num_runs: *mut usize) -> NeedleError;
    pub fn needle_hip_matcher_stats(matcher: *const NeedleHipMatcher, stats: *mut u64) -> NeedleError;

    pub fn needle_hip_crossmatcher_new(
        lanes: usize,
        max_items: usize,
        min_len: u32,
        threshold: u32,
        output: *mut *mut NeedleHipCrossMatcher,
    ) -> NeedleError;
    pub fn needle_hip_crossmatcher_new_regions(
        videos: usize,
        regions: usize,
        max_items: *const usize,
        min_len: *const u32,
        threshold: u32,
        output: *mut *mut NeedleHipCrossMatcher,
    ) -> NeedleError;
    pub fn needle_hip_crossmatcher_free(matcher: *mut NeedleHipCrossMatcher);
    pub fn needle_hip_crossmatcher_feed(matcher: *mut NeedleHipCrossMatcher, items: *const *const u32, num_items: *const usize) -> NeedleError;
    pub fn needle_hip_crossmatcher_feed_from_feeder(matcher: *mut NeedleHipCrossMatcher, feeder: *mut NeedleHipFeeder) -> NeedleError;
    pub fn needle_hip_crossmatcher_finish(matcher: *mut NeedleHipCrossMatcher, lanes: *const usize, k: usize) -> NeedleError;
    pub fn needle_hip_crossmatcher_ready(matcher: *mut NeedleHipCrossMatcher, num_runs: *mut usize, complete: *mut bool) -> NeedleError;
    pub fn needle_hip_crossmatcher_lane(matcher: *mut NeedleHipCrossMatcher, lane: usize, items_fed: *mut u64, finished: *mut bool) -> NeedleError;
    pub fn needle_hip_crossmatcher_runs(matcher: *mut NeedleHipCrossMatcher, first: usize, count: usize, runs: *mut NeedleHipRun) -> NeedleError;
    pub fn needle_hip_crossmatcher_stats(matcher: *const NeedleHipCrossMatcher, stats: *mut u64) -> NeedleError;
    pub fn needle_hip_crossmatcher_state_bytes(lanes: usize, max_items: usize) -> usize;
    pub fn needle_hip_crossmatcher_state_bytes_regions(videos: usize, regions: usize, max_items: *const usize) -> usize;
    pub fn needle_hip_crossmatcher_shape(matcher: *const NeedleHipCrossMatcher, videos: *mut usize, regions: *mut usize) -> NeedleError;
    pub fn needle_hip_crossmatcher_new_resident(
        hashes: *const u32,
        num_hashes: usize,
        resident: *const NeedleHipSeq,
        num_resident: usize,
        videos: usize,
        regions: usize,
        max_items: *const usize,
        min_len: *const u32,
        threshold: u32,
        output: *mut *mut NeedleHipCrossMatcher,
    ) -> NeedleError;
    pub fn needle_hip_crossmatcher_state_bytes_resident(
        resident: *const NeedleHipSeq,
        num_resident: usize,
        videos: usize,
        regions: usize,
        max_items: *const usize,
    ) -> usize;
    pub fn needle_hip_crossmatcher_resident(matcher: *const NeedleHipCrossMatcher, num_resident: *mut usize) -> NeedleError;
    pub fn needle_hip_crossmatcher_new_grouped(
        hashes: *const u32,
        num_hashes: usize,
        resident: *const NeedleHipSeq,
        num_resident: usize,
        resident_groups: *const u32,
        videos: usize,
        groups: *const u32,
        regions: usize,
        max_items: *const usize,
        min_len: *const u32,
        threshold: u32,
        output: *mut *mut NeedleHipCrossMatcher,
    ) -> NeedleError;
    pub fn needle_hip_crossmatcher_state_bytes_grouped(
        resident: *const NeedleHipSeq,
        num_resident: usize,
        resident_groups: *const u32,
        videos: usize,
        groups: *const u32,
        regions: usize,
        max_items: *const usize,
    ) -> usize;
    pub fn needle_hip_crossmatcher_groups(matcher: *const NeedleHipCrossMatcher, labels: *mut u32, n: usize) -> NeedleError;
    pub fn needle_hip_host_free(ptr: *mut c_void);
    // compressed fingerprints: chromaprint's codec on the device
    pub fn needle_hip_fingerprint_compressed_bound(items: usize) -> usize;
    pub fn needle_hip_fingerprint_compress_host(
        items: *const u32,
        item_offsets: *const u64,
        count: usize,
        algorithm: c_int,
        blobs: *mut *mut u8,
        blob_offsets: *mut u64,
    ) -> NeedleError;
    pub fn needle_hip_fingerprint_decompress_host(
        blobs: *const u8,
        blob_offsets: *const u64,
        count: usize,
        items: *mut *mut u32,
        item_offsets: *mut u64,
        algorithms: *mut i32,
        status: *mut i32,
    ) -> NeedleError;
    pub fn needle_hip_feeder_compressed(feeder: *mut NeedleHipFeeder, lane: usize, algorithm: c_int, blob: *mut *mut u8, size: *mut usize) -> NeedleError;
    pub fn needle_hip_fingerprint_base64_encode(data: *const u8, size: usize, text: *mut *mut c_char, text_size: *mut usize) -> NeedleError;
    pub fn needle_hip_fingerprint_base64_decode(text: *const c_char, text_size: usize, data: *mut *mut u8, size: *mut usize) -> NeedleError;
    pub fn needle_hip_fingerprint_codec_tiles(compress_items: *mut usize, decompress_symbols: *mut usize) -> NeedleError;
    pub fn needle_hip_fingerprint_simhash(items: *const u32, count: usize, hash: *mut u32) -> NeedleError;
}
