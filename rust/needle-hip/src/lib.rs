//! The `needle::audio` surface on the MI355X path.
//!
//! `Analyzer`, `Comparator`, `FrameHashes` and `SearchResult` carry the method set of the reference's
//! structs (needle/src/audio/analyzer.rs:95-151,425; comparator.rs:65-147,524,637; data.rs:74-168), so code
//! written against `needle::audio` ports by changing the `use` line.  Two differences, both forced by the
//! boundary this build draws (FFmpeg is upstream of it): video files are RIFF/WAVE PCM, and `Analyzer::run_pcm`
//! exists for callers that decode themselves.
//!
//! UNTESTED — see Cargo.toml.
pub mod ffi;

use std::ffi::{CStr, CString};
use std::path::{Path, PathBuf};
use std::ptr;
use std::time::Duration;

/// needle::Error (needle/src/lib.rs:117-149), as far as it crosses the C ABI (needle-capi/src/lib.rs:121-134).
#[derive(Debug, Clone, PartialEq, Eq)]
pub struct Error {
    pub code: ffi::NeedleError,
    pub message: String,
}

impl std::fmt::Display for Error {
    fn fmt(&self, f: &mut std::fmt::Formatter<'_>) -> std::fmt::Result {
        write!(f, "{}", self.message)
    }
}
impl std::error::Error for Error {}

pub type Result<T> = std::result::Result<T, Error>;

fn check(code: ffi::NeedleError) -> Result<()> {
    if code == ffi::NeedleError::Ok {
        return Ok(());
    }
    // SAFETY: both functions return pointers to NUL-terminated strings owned by the library.
    let message = unsafe {
        let detail = ffi::needle_hip_last_error_message();
        if !detail.is_null() && *detail != 0 {
            CStr::from_ptr(detail).to_string_lossy().into_owned()
        } else {
            CStr::from_ptr(ffi::needle_error_to_str(code)).to_string_lossy().into_owned()
        }
    };
    Err(Error { code, message })
}

fn c_paths<P: AsRef<Path>>(paths: &[P]) -> Result<(Vec<CString>, Vec<*const std::os::raw::c_char>)> {
    let owned = paths
        .iter()
        .map(|p| {
            CString::new(p.as_ref().to_string_lossy().as_bytes()).map_err(|_| Error {
                code: ffi::NeedleError::InvalidUtf8String,
                message: "path contains a NUL byte".into(),
            })
        })
        .collect::<Result<Vec<_>>>()?;
    let raw = owned.iter().map(|s| s.as_ptr()).collect();
    Ok((owned, raw))
}

pub const DEFAULT_HASH_MATCH_THRESHOLD: u16 = 10; // audio/mod.rs:14
pub const DEFAULT_OPENING_SEARCH_PERCENTAGE: f32 = 0.50;
pub const DEFAULT_ENDING_SEARCH_PERCENTAGE: f32 = 0.25;
pub const DEFAULT_MIN_OPENING_DURATION: u16 = 20;
pub const DEFAULT_MIN_ENDING_DURATION: u16 = 20;
pub const DEFAULT_HASH_DURATION: f32 = 0.3;
pub const DEFAULT_OPENING_AND_ENDING_TIME_PADDING: f32 = 0.0;

/// data.rs:74-80.  Owns a library-side `FrameHashes`.
pub struct FrameHashes {
    raw: *mut ffi::FrameHashes,
    opening: Vec<(u32, Duration)>,
    ending: Vec<(u32, Duration)>,
    md5: String,
}

// The handle is plain heap data inside the library, not tied to a thread.
unsafe impl Send for FrameHashes {}

impl FrameHashes {
    /// Takes ownership of `raw`.
    unsafe fn from_raw(raw: *mut ffi::FrameHashes) -> Result<Self> {
        let side = |ending: bool| -> Result<Vec<(u32, Duration)>> {
            let n = ffi::needle_hip_frame_hashes_len(raw, ending);
            let (mut h, mut t) = (vec![0u32; n], vec![0u64; n]);
            check(ffi::needle_hip_frame_hashes_copy(raw, ending, h.as_mut_ptr(), t.as_mut_ptr(), n))?;
            Ok(h.into_iter().zip(t.into_iter().map(Duration::from_nanos)).collect())
        };
        let md5 = CStr::from_ptr(ffi::needle_hip_frame_hashes_md5(raw)).to_string_lossy().into_owned();
        Ok(FrameHashes { raw, opening: side(false)?, ending: side(true)?, md5 })
    }

    /// Copies a handle the analyzer still owns (needle_audio_analyzer_get_frame_hashes lends it).
    unsafe fn clone_borrowed(borrowed: *const ffi::FrameHashes) -> Result<Self> {
        let side = |ending: bool| -> Result<(Vec<u32>, Vec<u64>)> {
            let n = ffi::needle_hip_frame_hashes_len(borrowed, ending);
            let (mut h, mut t) = (vec![0u32; n], vec![0u64; n]);
            check(ffi::needle_hip_frame_hashes_copy(borrowed, ending, h.as_mut_ptr(), t.as_mut_ptr(), n))?;
            Ok((h, t))
        };
        let (oh, ot) = side(false)?;
        let (eh, et) = side(true)?;
        let mut raw = ptr::null_mut();
        check(ffi::needle_hip_frame_hashes_new(
            oh.as_ptr(),
            ot.as_ptr(),
            oh.len(),
            eh.as_ptr(),
            et.as_ptr(),
            eh.len(),
            ffi::needle_hip_frame_hashes_hash_duration_ns(borrowed),
            ffi::needle_hip_frame_hashes_md5(borrowed),
            &mut raw,
        ))?;
        Self::from_raw(raw)
    }

    /// data.rs:104-115: `<video>.needle.dat` next to the video.
    pub fn from_path(path: impl AsRef<Path>) -> Result<Self> {
        let (_owned, raw_paths) = c_paths(&[path])?;
        let mut raw = ptr::null_mut();
        // SAFETY: valid NUL-terminated path, valid out pointer.
        unsafe {
            check(ffi::needle_hip_frame_hashes_read(raw_paths[0], &mut raw))?;
            Self::from_raw(raw)
        }
    }

    pub fn to_path(&self, path: impl AsRef<Path>) -> Result<()> {
        let (_owned, raw_paths) = c_paths(&[path])?;
        unsafe { check(ffi::needle_hip_frame_hashes_write(self.raw, raw_paths[0])) }
    }

    pub fn opening_data(&self) -> &[(u32, Duration)] {
        &self.opening
    }
    pub fn ending_data(&self) -> &[(u32, Duration)] {
        &self.ending
    }
    pub fn hash_duration(&self) -> Duration {
        Duration::from_nanos(unsafe { ffi::needle_hip_frame_hashes_hash_duration_ns(self.raw) })
    }
    pub fn md5(&self) -> &str {
        &self.md5
    }
}

impl Drop for FrameHashes {
    fn drop(&mut self) {
        unsafe { ffi::needle_hip_frame_hashes_free(self.raw) }
    }
}

/// analyzer.rs:77-151.
pub struct Analyzer<P: AsRef<Path>> {
    videos: Vec<P>,
    opening_search_percentage: f32,
    ending_search_percentage: f32,
    include_endings: bool,
    threaded_decoding: bool,
    force: bool,
}

impl<P: AsRef<Path>> Default for Analyzer<P> {
    fn default() -> Self {
        Analyzer {
            videos: Vec::new(),
            opening_search_percentage: DEFAULT_OPENING_SEARCH_PERCENTAGE,
            ending_search_percentage: DEFAULT_ENDING_SEARCH_PERCENTAGE,
            include_endings: false,
            threaded_decoding: false,
            force: false,
        }
    }
}

impl<P: AsRef<Path>> Analyzer<P> {
    pub fn from_files(videos: impl Into<Vec<P>>, threaded_decoding: bool, force: bool) -> Self {
        Analyzer { videos: videos.into(), threaded_decoding, force, ..Default::default() }
    }
    pub fn videos(&self) -> &[P] {
        &self.videos
    }
    pub fn with_opening_search_percentage(mut self, v: f32) -> Self {
        self.opening_search_percentage = v;
        self
    }
    pub fn with_ending_search_percentage(mut self, v: f32) -> Self {
        self.ending_search_percentage = v;
        self
    }
    pub fn with_include_endings(mut self, v: bool) -> Self {
        self.include_endings = v;
        self
    }
    pub fn with_threaded_decoding(mut self, v: bool) -> Self {
        self.threaded_decoding = v;
        self
    }
    pub fn with_force(mut self, v: bool) -> Self {
        self.force = v;
        self
    }

    fn handle(&self) -> Result<*mut ffi::NeedleAudioAnalyzer> {
        let (_owned, raw) = c_paths(&self.videos)?;
        let mut out = ptr::null_mut();
        // SAFETY: `raw` outlives the call; the library copies the strings (needle-capi/src/lib.rs:373-409).
        unsafe {
            check(ffi::needle_audio_analyzer_new(
                raw.as_ptr(),
                raw.len(),
                self.opening_search_percentage,
                self.ending_search_percentage,
                self.include_endings,
                self.threaded_decoding,
                self.force,
                &mut out,
            ))?;
        }
        Ok(out)
    }

    fn collect(&self, handle: *mut ffi::NeedleAudioAnalyzer) -> Result<Vec<FrameHashes>> {
        (0..self.videos.len())
            .map(|i| unsafe {
                let mut fh = ptr::null();
                check(ffi::needle_audio_analyzer_get_frame_hashes(handle, i, &mut fh))?;
                FrameHashes::clone_borrowed(fh)
            })
            .collect()
    }

    /// analyzer.rs:425-455.  `threading` is accepted for signature parity: the batch is one GPU launch.
    pub fn run(&self, hash_duration: Duration, persist: bool, threading: bool) -> Result<Vec<FrameHashes>> {
        let handle = self.handle()?;
        let result = unsafe {
            check(ffi::needle_audio_analyzer_run(handle, hash_duration.as_secs_f32(), persist, threading))
        }
        .and_then(|_| self.collect(handle));
        unsafe { ffi::needle_audio_analyzer_free(handle) };
        result
    }

    /// Extension: the decoded stream of every video, interleaved s16 at `sample_rate` (any rate; it is
    /// resampled to chromaprint's 11025 Hz on the device), instead of a file to decode.
    pub fn run_pcm(
        &self,
        pcm: &[&[i16]],
        channels: i32,
        sample_rate: i32,
        hash_duration: Duration,
        persist: bool,
    ) -> Result<Vec<FrameHashes>> {
        assert_eq!(pcm.len(), self.videos.len(), "one PCM stream per video");
        let ptrs: Vec<*const i16> = pcm.iter().map(|s| s.as_ptr()).collect();
        let lens: Vec<usize> = pcm.iter().map(|s| s.len()).collect();
        let handle = self.handle()?;
        let result = unsafe {
            check(ffi::needle_hip_analyzer_run_pcm(
                handle,
                ptrs.as_ptr(),
                lens.as_ptr(),
                channels,
                sample_rate,
                hash_duration.as_secs_f32(),
                persist,
            ))
        }
        .and_then(|_| self.collect(handle));
        unsafe { ffi::needle_audio_analyzer_free(handle) };
        result
    }

    /// `run_pcm` with the samples as the decoder hands them over (u8 / i16 / i32 / f32 / f64), converted on the device
    /// (`needle_hip_analyzer_run_pcm_format`).  `planar`: `pcm` holds `channels` planes per video, one after the other;
    /// otherwise one interleaved slice per video.
    pub fn run_pcm_format<T: Sample>(
        &self,
        pcm: &[&[T]],
        planar: bool,
        channels: i32,
        sample_rate: i32,
        hash_duration: Duration,
        persist: bool,
    ) -> Result<Vec<FrameHashes>> {
        let planes = if planar { channels.max(1) as usize } else { 1 };
        assert_eq!(pcm.len(), self.videos.len() * planes, "one slice per plane of every video");
        let ptrs: Vec<*const std::os::raw::c_void> = pcm.iter().map(|s| s.as_ptr() as *const _).collect();
        let lens: Vec<usize> = pcm.chunks(planes).map(|s| s.iter().map(|p| p.len()).sum()).collect();
        let format = if planar { T::PLANAR } else { T::INTERLEAVED };
        let handle = self.handle()?;
        let result = unsafe {
            check(ffi::needle_hip_analyzer_run_pcm_format(
                handle,
                ptrs.as_ptr(),
                lens.as_ptr(),
                channels,
                sample_rate,
                format as i32,
                hash_duration.as_secs_f32(),
                persist,
            ))
        }
        .and_then(|_| self.collect(handle));
        unsafe { ffi::needle_audio_analyzer_free(handle) };
        result
    }

    /// `run_pcm_format` with a format per stream and, optionally, a mix per stream (`channels == 0`: the plain average)
    /// in one device pass (`needle_hip_analyzer_run_pcm_formats`).  `planes` is the concatenation of every stream's
    /// planes as raw pointers -- one for an interleaved stream, `channels` for a planar one -- and `num_values[i]` counts
    /// stream i's values over all its channels.
    ///
    /// # Safety
    /// Every plane must hold the samples `formats` and `num_values` describe.
    pub unsafe fn run_pcm_formats(
        &self,
        planes: &[*const std::os::raw::c_void],
        num_values: &[usize],
        formats: &[ffi::NeedleHipLaneFormat],
        mixes: Option<&[ffi::NeedleHipChannelMix]>,
        hash_duration: Duration,
        persist: bool,
    ) -> Result<Vec<FrameHashes>> {
        assert!(num_values.len() == self.videos.len() && formats.len() == self.videos.len());
        assert!(mixes.map_or(true, |m| m.len() == self.videos.len()));
        let expected: usize = formats.iter().map(|f| if f.format >= 5 { f.channels.max(1) as usize } else { 1 }).sum();
        assert_eq!(planes.len(), expected, "one pointer per plane of every stream");
        let handle = self.handle()?;
        let result = check(ffi::needle_hip_analyzer_run_pcm_formats(
            handle,
            planes.as_ptr(),
            num_values.as_ptr(),
            formats.as_ptr(),
            mixes.map_or(std::ptr::null(), |m| m.as_ptr()),
            hash_duration.as_secs_f32(),
            persist,
        ))
        .and_then(|_| self.collect(handle));
        ffi::needle_audio_analyzer_free(handle);
        result
    }
}

/// comparator.rs:65-69.  The reference keeps the fields private; accessors are an extension.
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct SearchResult {
    opening: Option<(Duration, Duration)>,
    ending: Option<(Duration, Duration)>,
}

impl SearchResult {
    pub fn opening(&self) -> Option<(Duration, Duration)> {
        self.opening
    }
    pub fn ending(&self) -> Option<(Duration, Duration)> {
        self.ending
    }
}

pub use ffi::NeedleHipMatchEvidence as MatchEvidence;

/// `NeedleHipSearchEvidence` with a region that has no match (`partner == u32::MAX`) as `None`.
#[derive(Clone, Copy, Debug, Default, PartialEq)]
pub struct SearchEvidence {
    pub opening: Option<MatchEvidence>,
    pub ending: Option<MatchEvidence>,
}

impl From<ffi::NeedleHipSearchEvidence> for SearchEvidence {
    fn from(e: ffi::NeedleHipSearchEvidence) -> Self {
        let some = |m: MatchEvidence| (m.partner != u32::MAX).then_some(m);
        SearchEvidence { opening: some(e.opening()), ending: some(e.ending()) }
    }
}

/// comparator.rs:74-147.
pub struct Comparator<P: AsRef<Path>> {
    videos: Vec<P>,
    include_endings: bool,
    hash_match_threshold: u32,
    min_opening_duration: Duration,
    min_ending_duration: Duration,
    time_padding: Duration,
}

impl<P: AsRef<Path>> Default for Comparator<P> {
    fn default() -> Self {
        Comparator {
            videos: Vec::new(),
            include_endings: false,
            hash_match_threshold: DEFAULT_HASH_MATCH_THRESHOLD as u32,
            min_opening_duration: Duration::from_secs(DEFAULT_MIN_OPENING_DURATION as u64),
            min_ending_duration: Duration::from_secs(DEFAULT_MIN_ENDING_DURATION as u64),
            time_padding: Duration::from_secs_f32(DEFAULT_OPENING_AND_ENDING_TIME_PADDING),
        }
    }
}

impl<P: AsRef<Path>> From<Analyzer<P>> for Comparator<P> {
    fn from(analyzer: Analyzer<P>) -> Self {
        Comparator { videos: analyzer.videos, ..Default::default() } // comparator.rs:96-104: the path list only
    }
}

impl<P: AsRef<Path>> Comparator<P> {
    pub fn from_files(videos: impl Into<Vec<P>>) -> Self {
        Comparator { videos: videos.into(), ..Default::default() }
    }
    pub fn videos(&self) -> &[P] {
        &self.videos
    }
    pub fn with_include_endings(mut self, v: bool) -> Self {
        self.include_endings = v;
        self
    }
    pub fn with_hash_match_threshold(mut self, v: u32) -> Self {
        self.hash_match_threshold = v;
        self
    }
    pub fn with_min_opening_duration(mut self, v: Duration) -> Self {
        self.min_opening_duration = v;
        self
    }
    pub fn with_min_ending_duration(mut self, v: Duration) -> Self {
        self.min_ending_duration = v;
        self
    }
    pub fn with_time_padding(mut self, v: Duration) -> Self {
        self.time_padding = v;
        self
    }

    fn handle(&self) -> Result<*const ffi::NeedleAudioComparator> {
        let (_owned, raw) = c_paths(&self.videos)?;
        let mut out = ptr::null();
        // The C constructor takes whole seconds as u16 (needle-capi/src/lib.rs:556-599), like the CLI does.
        unsafe {
            check(ffi::needle_audio_comparator_new(
                raw.as_ptr(),
                raw.len(),
                self.include_endings,
                self.hash_match_threshold.min(u16::MAX as u32) as u16,
                self.min_opening_duration.as_secs().min(u16::MAX as u64) as u16,
                self.min_ending_duration.as_secs().min(u16::MAX as u64) as u16,
                self.time_padding.as_secs_f32(),
                &mut out,
            ))?;
        }
        Ok(out)
    }

    /// The host epilogue alone, with the evidence beside every result (`needle_hip_comparator_results_from_runs_evidence`):
    /// from a complete run list of all pairs to one (result, evidence) per video of `[first_video, first_video +
    /// video_count)`; the other slots are `None` / no match.  No device work.
    pub fn results_from_runs_evidence(
        &self,
        frame_hashes: &[FrameHashes],
        runs: &[ffi::NeedleHipRun],
        first_video: usize,
        video_count: usize,
    ) -> Result<Vec<(Option<SearchResult>, SearchEvidence)>> {
        let handle = self.handle()?;
        let raw: Vec<*const ffi::FrameHashes> = frame_hashes.iter().map(|f| f.raw as *const _).collect();
        let mut results = vec![ffi::NeedleHipSearchResult::default(); raw.len()];
        let mut evidence = vec![ffi::NeedleHipSearchEvidence::default(); raw.len()];
        let status = unsafe {
            check(ffi::needle_hip_comparator_results_from_runs_evidence(
                handle,
                raw.as_ptr(),
                raw.len(),
                runs.as_ptr(),
                runs.len(),
                first_video,
                video_count,
                results.as_mut_ptr(),
                evidence.as_mut_ptr(),
            ))
        };
        unsafe { ffi::needle_audio_comparator_free(handle) };
        status?;
        let span = |a: u64, b: u64| (Duration::from_nanos(a), Duration::from_nanos(b));
        Ok(results
            .into_iter()
            .zip(evidence)
            .map(|(r, e)| {
                let result = r.has_result.then(|| SearchResult {
                    opening: r.has_opening.then(|| span(r.opening_start_ns, r.opening_end_ns)),
                    ending: r.has_ending.then(|| span(r.ending_start_ns, r.ending_end_ns)),
                });
                (result, SearchEvidence::from(e))
            })
            .collect())
    }

    /// `run_with_frame_hashes` over groups of videos (`needle_hip_comparator_run_with_frame_hashes_grouped`): `groups` has a
    /// label per video, and only videos of equal label are compared.  One entry per video, `None` where it matched nothing
    /// (a video alone in its group always).
    pub fn run_with_frame_hashes_grouped(
        &self,
        frame_hashes: &[FrameHashes],
        groups: &[u32],
        display: bool,
        use_skip_files: bool,
        write_skip_files: bool,
    ) -> Result<Vec<Option<SearchResult>>> {
        if groups.len() != frame_hashes.len() {
            return Err(Error {
                code: ffi::NeedleError::InvalidArgument,
                message: "grouped search: one group label per video".into(),
            });
        }
        let handle = self.handle()?;
        let raw: Vec<*const ffi::FrameHashes> = frame_hashes.iter().map(|f| f.raw as *const _).collect();
        let mut results = vec![ffi::NeedleHipSearchResult::default(); raw.len()];
        let status = unsafe {
            check(ffi::needle_hip_comparator_run_with_frame_hashes_grouped(
                handle,
                raw.as_ptr(),
                raw.len(),
                groups.as_ptr(),
                display,
                use_skip_files,
                write_skip_files,
                results.as_mut_ptr(),
            ))
        };
        unsafe { ffi::needle_audio_comparator_free(handle) };
        status?;
        Ok(results.into_iter().map(optional_result).collect())
    }

    /// The host epilogue alone over a grouped run list (`needle_hip_comparator_results_from_runs_grouped`; `problem` =
    /// grouped pair id * regions + region, see [`group_pairs`]).  No device work.
    pub fn results_from_runs_grouped(
        &self,
        frame_hashes: &[FrameHashes],
        groups: &[u32],
        runs: &[ffi::NeedleHipRun],
    ) -> Result<Vec<Option<SearchResult>>> {
        if groups.len() != frame_hashes.len() {
            return Err(Error {
                code: ffi::NeedleError::InvalidArgument,
                message: "grouped search: one group label per video".into(),
            });
        }
        let handle = self.handle()?;
        let raw: Vec<*const ffi::FrameHashes> = frame_hashes.iter().map(|f| f.raw as *const _).collect();
        let mut results = vec![ffi::NeedleHipSearchResult::default(); raw.len()];
        let status = unsafe {
            check(ffi::needle_hip_comparator_results_from_runs_grouped(
                handle,
                raw.as_ptr(),
                raw.len(),
                groups.as_ptr(),
                runs.as_ptr(),
                runs.len(),
                results.as_mut_ptr(),
            ))
        };
        unsafe { ffi::needle_audio_comparator_free(handle) };
        status?;
        Ok(results.into_iter().map(optional_result).collect())
    }

    /// The file-based `run` over groups of videos (`needle_hip_comparator_run_grouped`): `groups` is parallel to the
    /// comparator's paths.
    pub fn run_grouped(&self, groups: &[u32], analyze: bool, display: bool, use_skip_files: bool, write_skip_files: bool) -> Result<()> {
        let handle = self.handle()?;
        let status = unsafe {
            check(ffi::needle_hip_comparator_run_grouped(
                handle,
                groups.as_ptr(),
                groups.len(),
                analyze,
                display,
                use_skip_files,
                write_skip_files,
            ))
        };
        unsafe { ffi::needle_audio_comparator_free(handle) };
        status
    }

    /// comparator.rs:524-629.  One entry per video that matched something, in video order (`:608-617`).
    pub fn run_with_frame_hashes(
        &self,
        frame_hashes: Vec<FrameHashes>,
        display: bool,
        use_skip_files: bool,
        write_skip_files: bool,
        _threading: bool,
    ) -> Result<Vec<SearchResult>> {
        let handle = self.handle()?;
        let raw: Vec<*const ffi::FrameHashes> = frame_hashes.iter().map(|f| f.raw as *const _).collect();
        let mut results = vec![ffi::NeedleHipSearchResult::default(); raw.len()];
        let status = unsafe {
            check(ffi::needle_hip_comparator_run_with_frame_hashes(
                handle,
                raw.as_ptr(),
                raw.len(),
                display,
                use_skip_files,
                write_skip_files,
                results.as_mut_ptr(),
            ))
        };
        unsafe { ffi::needle_audio_comparator_free(handle) };
        status?;
        let span = |a: u64, b: u64| (Duration::from_nanos(a), Duration::from_nanos(b));
        Ok(results
            .into_iter()
            .filter(|r| r.has_result)
            .map(|r| SearchResult {
                opening: r.has_opening.then(|| span(r.opening_start_ns, r.opening_end_ns)),
                ending: r.has_ending.then(|| span(r.ending_start_ns, r.ending_end_ns)),
            })
            .collect())
    }

    /// comparator.rs:637-660: frame hashes from disk (or analyzed in place), then `run_with_frame_hashes`.
    /// Results are observable through stdout / skip files, as upstream (needle-capi/src/lib.rs:634).
    pub fn run(
        &self,
        analyze: bool,
        display: bool,
        use_skip_files: bool,
        write_skip_files: bool,
        threading: bool,
    ) -> Result<()> {
        let handle = self.handle()?;
        let status = unsafe {
            check(ffi::needle_audio_comparator_run(handle, analyze, display, use_skip_files, write_skip_files, threading))
        };
        unsafe { ffi::needle_audio_comparator_free(handle) };
        status
    }
}

/// Streaming fingerprinter (`needle_hip_feeder_*`): chromaprint's start / feed / finish, batched over lanes -- one per
/// decoder -- with the per-lane state on the device.  After `finish` a lane's items are bit for bit those of the one-shot
/// path over the concatenation of its chunks.
pub struct Feeder {
    raw: *mut ffi::NeedleHipFeeder,
    lanes: usize,
    planes: usize,
    formats: Option<Vec<LaneFormat>>, // `with_formats`: every lane's own, kept up to date by `reset_format` / `switch_format`
}

/// `(channels, sample rate, NeedleHipSampleFormat)` of a feeder lane.
pub use ffi::NeedleHipLaneFormat as LaneFormat;
/// One segment of a lane's stream: a format and the frames fed in it (`Feeder::switch_format`).
pub use ffi::NeedleHipSegment as Segment;

fn format_planes(f: &LaneFormat) -> usize {
    if f.format >= 5 { f.channels.max(1) as usize } else { 1 }
}

unsafe impl Send for Feeder {}

impl Feeder {
    /// `T` and `planar` give the sample format, as in `Analyzer::run_pcm_format`.
    pub fn new<T: Sample>(lanes: usize, channels: i32, sample_rate: i32, planar: bool, step: u32) -> Result<Self> {
        let format = if planar { T::PLANAR } else { T::INTERLEAVED };
        let mut raw = ptr::null_mut();
        unsafe { check(ffi::needle_hip_feeder_new(lanes, channels, sample_rate, format as i32, step, &mut raw))? };
        Ok(Feeder { raw, lanes, planes: if planar { channels.max(1) as usize } else { 1 }, formats: None })
    }

    /// One lane per format (`needle_hip_feeder_new_lanes`): a season whose episodes differ in channel count, rate and
    /// sample format in one feeder.  Every lane is down-mixed to mono as it lands; the items are the one-shot path's.
    /// Such a feeder is fed with `feed_lanes`.
    pub fn with_formats(formats: &[LaneFormat], step: u32) -> Result<Self> {
        let mut raw = ptr::null_mut();
        unsafe { check(ffi::needle_hip_feeder_new_lanes(formats.as_ptr(), formats.len(), step, &mut raw))? };
        Ok(Feeder { raw, lanes: formats.len(), planes: 0, formats: Some(formats.to_vec()) })
    }

    pub fn lane_format(&self, lane: usize) -> Result<LaneFormat> {
        let mut f = LaneFormat::default();
        unsafe { check(ffi::needle_hip_feeder_lane_format(self.raw, lane, &mut f))? };
        Ok(f)
    }

    /// `lanes[j]` folds its channels with `mixes[j]` (`ChannelMix::default()`, channels 0: the plain average again);
    /// only on a feeder made by `with_formats`, and only lanes that hold no samples (`needle_hip_feeder_set_lane_mix`).
    pub fn set_lane_mix(&mut self, lanes: &[usize], mixes: &[ChannelMix]) -> Result<()> {
        assert_eq!(lanes.len(), mixes.len(), "one mix per lane");
        unsafe { check(ffi::needle_hip_feeder_set_lane_mix(self.raw, lanes.as_ptr(), mixes.as_ptr(), lanes.len())) }
    }

    /// `lanes[j]` starts a new stream in `formats[j]`; only on a feeder made by `with_formats`.
    pub fn reset_format(&mut self, lanes: &[usize], formats: &[LaneFormat]) -> Result<()> {
        assert_eq!(lanes.len(), formats.len(), "one format per lane");
        unsafe { check(ffi::needle_hip_feeder_reset_format(self.raw, lanes.as_ptr(), formats.as_ptr(), lanes.len()))? };
        if let Some(mine) = self.formats.as_mut() {
            for (&lane, f) in lanes.iter().zip(formats) {
                mine[lane] = *f;
            }
        }
        Ok(())
    }

    /// `lanes[j]` ends its current segment and continues ITS SAME STREAM in `formats[j]`, folded by `mixes[j]` (`None`, or
    /// a mix of 0 channels: the plain average): a decoder that reports another rate, layout or sample format in
    /// mid-stream.  The fingerprint goes on across the change; only on a feeder made by `with_formats`.
    pub fn switch_format(&mut self, lanes: &[usize], formats: &[LaneFormat], mixes: Option<&[ChannelMix]>) -> Result<()> {
        assert_eq!(lanes.len(), formats.len(), "one format per lane");
        assert!(mixes.map_or(true, |m| m.len() == lanes.len()), "one mix per lane");
        let mixes = mixes.map_or(ptr::null(), |m| m.as_ptr());
        unsafe { check(ffi::needle_hip_feeder_switch_format(self.raw, lanes.as_ptr(), formats.as_ptr(), mixes, lanes.len()))? };
        if let Some(mine) = self.formats.as_mut() {
            for (&lane, f) in lanes.iter().zip(formats) {
                mine[lane] = *f;
            }
        }
        Ok(())
    }

    /// The segments of the lane's current stream, the open one last.
    pub fn lane_segments(&self, lane: usize) -> Result<Vec<Segment>> {
        let mut count = 0usize;
        unsafe { check(ffi::needle_hip_feeder_lane_segments(self.raw, lane, ptr::null_mut(), 0, &mut count))? };
        let mut out = vec![Segment::default(); count];
        unsafe { check(ffi::needle_hip_feeder_lane_segments(self.raw, lane, out.as_mut_ptr(), out.len(), &mut count))? };
        out.truncate(count);
        Ok(out)
    }

    /// Kept items a lane holds after these segments, the last one open unless `finished` (host arithmetic, no device).
    pub fn num_ready_segments(segments: &[Segment], step: u32, finished: bool) -> usize {
        unsafe { ffi::needle_hip_feeder_num_ready_segments(segments.as_ptr(), segments.len(), step, finished) }
    }

    /// The feed of a `with_formats` feeder, whose lanes differ in sample type: per lane the raw bytes of its planes (1 of
    /// an interleaved lane, `channels` of a planar one; an empty slice is nothing for that lane), aligned to one sample.
    pub fn feed_lanes(&mut self, pcm: &[&[&[u8]]]) -> Result<()> {
        let formats = self.formats.as_ref().expect("feed_lanes is the feed of a with_formats feeder");
        assert_eq!(pcm.len(), self.lanes, "one entry per lane");
        let (mut ptrs, mut lens) = (Vec::new(), Vec::with_capacity(self.lanes));
        for (planes, f) in pcm.iter().zip(formats) {
            assert_eq!(planes.len(), format_planes(f), "one slice per plane of the lane");
            let width = [1usize, 2, 4, 4, 8][(f.format % 5) as usize];
            ptrs.extend(planes.iter().map(|s| s.as_ptr() as *const std::os::raw::c_void));
            lens.push(planes.iter().map(|p| p.len() / width).sum::<usize>());
        }
        unsafe { check(ffi::needle_hip_feeder_feed(self.raw, ptrs.as_ptr(), lens.as_ptr())) }
    }

    /// What every lane has decoded since the last feed: one slice per lane (planar: `channels` planes per lane, one after
    /// the other); an empty slice is nothing for that lane.  The slices may be reused on return.
    pub fn feed<T: Sample>(&mut self, pcm: &[&[T]]) -> Result<()> {
        assert!(self.formats.is_none(), "a with_formats feeder is fed with feed_lanes");
        assert_eq!(pcm.len(), self.lanes * self.planes, "one slice per plane of every lane");
        let ptrs: Vec<*const std::os::raw::c_void> = pcm.iter().map(|s| s.as_ptr() as *const _).collect();
        let lens: Vec<usize> = pcm.chunks(self.planes).map(|s| s.iter().map(|p| p.len()).sum()).collect();
        unsafe { check(ffi::needle_hip_feeder_feed(self.raw, ptrs.as_ptr(), lens.as_ptr())) }
    }

    /// `None`: every unfinished lane.
    pub fn finish(&mut self, lanes: Option<&[usize]>) -> Result<()> {
        let (p, k) = lanes.map_or((ptr::null(), 0), |l| (l.as_ptr(), l.len()));
        unsafe { check(ffi::needle_hip_feeder_finish(self.raw, p, k)) }
    }

    /// The lanes start new streams (`None`: every lane).
    pub fn reset(&mut self, lanes: Option<&[usize]>) -> Result<()> {
        let (p, k) = lanes.map_or((ptr::null(), 0), |l| (l.as_ptr(), l.len()));
        unsafe { check(ffi::needle_hip_feeder_reset(self.raw, p, k)) }
    }

    /// `(kept items, samples per channel fed, finished)` of a lane; waits for outstanding device work.
    pub fn ready(&mut self, lane: usize) -> Result<(usize, u64, bool)> {
        let (mut kept, mut fed, mut finished) = (0usize, 0u64, false);
        unsafe { check(ffi::needle_hip_feeder_ready(self.raw, lane, &mut kept, &mut fed, &mut finished))? };
        Ok((kept, fed, finished))
    }

    pub fn items(&mut self, lane: usize, first: usize, count: usize) -> Result<Vec<u32>> {
        let mut out = vec![0u32; count];
        unsafe { check(ffi::needle_hip_feeder_items(self.raw, lane, first, count, out.as_mut_ptr()))? };
        Ok(out)
    }

    /// A finished lane's kept items in chromaprint's compressed form; [`base64_encode`] gives the string `fpcalc` prints.
    pub fn compressed(&mut self, lane: usize, algorithm: i32) -> Result<Vec<u8>> {
        let (mut blob, mut size) = (ptr::null_mut(), 0usize);
        unsafe {
            check(ffi::needle_hip_feeder_compressed(self.raw, lane, algorithm, &mut blob, &mut size))?;
            Ok(take_host(blob, size))
        }
    }

    /// The `FrameHashes` of one video from its finished opening lane and, optionally, its ending lane with the seek offset of
    /// the ending window (analyzer.rs:314-318).
    pub fn frame_hashes(&mut self, opening_lane: usize, ending: Option<(usize, Duration)>, hash_duration: Duration, md5: &str) -> Result<FrameHashes> {
        let md5 = CString::new(md5).map_err(|_| Error { code: ffi::NeedleError::InvalidUtf8String, message: "md5 holds a NUL".into() })?;
        let (lane, seek) = ending.map_or((usize::MAX, 0u64), |(l, d)| (l, d.as_nanos() as u64));
        let mut raw = ptr::null_mut();
        unsafe {
            check(ffi::needle_hip_feeder_frame_hashes(self.raw, opening_lane, lane, seek, hash_duration.as_secs_f32(), md5.as_ptr(), &mut raw))?;
            FrameHashes::from_raw(raw)
        }
    }

    /// `(the most state one lane has carried from one feed to the next, high-water of one feed's staging)` in bytes.
    pub fn state_bytes(&self) -> Result<(u64, u64)> {
        let mut bytes = [0u64; 2];
        unsafe { check(ffi::needle_hip_feeder_state_bytes(self.raw, bytes.as_mut_ptr()))? };
        Ok((bytes[0], bytes[1]))
    }

    /// Switches the audit of the f32 first pass that travels with the stream; only while no lane holds samples.
    pub fn set_audit(&mut self, on: bool) -> Result<()> {
        unsafe { check(ffi::needle_hip_feeder_set_audit(self.raw, on)) }
    }

    /// The audit of a lane's current stream so far, or of all lanes (`None`: counts summed, maxima taken):
    /// `mismatches` and `accepted_mismatches` must be 0 (`needle_hip_feeder_audit`).  Waits for the library stream.
    pub fn audit(&mut self, lane: Option<usize>) -> Result<ffi::NeedleHipCertAudit> {
        let mut a = ffi::NeedleHipCertAudit::default();
        unsafe { check(ffi::needle_hip_feeder_audit(self.raw, lane.unwrap_or(usize::MAX), &mut a))? };
        Ok(a)
    }

    /// Kept items a lane holds after that many samples (host arithmetic, no device).
    pub fn num_ready(samples_per_channel_fed: u64, sample_rate: i32, channels: i32, step: u32, finished: bool) -> usize {
        unsafe { ffi::needle_hip_feeder_num_ready(samples_per_channel_fed, sample_rate, channels, step, finished) }
    }
}

impl Drop for Feeder {
    fn drop(&mut self) {
        unsafe { ffi::needle_hip_feeder_free(self.raw) };
    }
}

/// Streaming comparator (`needle_hip_matcher_*`): the search half of the streaming path.  The sources stay on the device;
/// every lane is a destination sequence that arrives in chunks; a feed evaluates the cells of its new columns only.  After
/// `finish` a lane's runs equal those of the one-shot scan over the concatenation of its chunks.
pub struct Matcher {
    raw: *mut ffi::NeedleHipMatcher,
    lanes: usize,
}

unsafe impl Send for Matcher {}

impl Matcher {
    /// One `(hashes, min_len)` per source.  Fails without a HIP device: the sources are uploaded here.
    pub fn new(sources: &[(&[u32], u32)], lanes: usize, threshold: u32) -> Result<Self> {
        let mut arena: Vec<u32> = Vec::new();
        let mut seqs = Vec::with_capacity(sources.len());
        let mut min_len = Vec::with_capacity(sources.len());
        for (hashes, min) in sources {
            seqs.push(ffi::NeedleHipSeq { offset: arena.len() as u32, len: hashes.len() as u32 });
            arena.extend_from_slice(hashes);
            min_len.push(*min);
        }
        let mut raw = ptr::null_mut();
        unsafe {
            check(ffi::needle_hip_matcher_new(arena.as_ptr(), arena.len(), seqs.as_ptr(), min_len.as_ptr(), seqs.len(), lanes, threshold, &mut raw))?;
        }
        Ok(Matcher { raw, lanes })
    }

    /// Openings against openings, endings against endings: source `s` is in region `s % regions`, lane `l` in region
    /// `l % regions`, and a lane meets its own region's sources only.  A `min_len` of 0 is allowed: that source has no cells.
    pub fn with_regions(sources: &[(&[u32], u32)], regions: usize, lanes: usize, threshold: u32) -> Result<Self> {
        let mut arena: Vec<u32> = Vec::new();
        let mut seqs = Vec::with_capacity(sources.len());
        let mut min_len = Vec::with_capacity(sources.len());
        for (hashes, min) in sources {
            seqs.push(ffi::NeedleHipSeq { offset: arena.len() as u32, len: hashes.len() as u32 });
            arena.extend_from_slice(hashes);
            min_len.push(*min);
        }
        let mut raw = ptr::null_mut();
        unsafe {
            check(ffi::needle_hip_matcher_new_regions(
                arena.as_ptr(), arena.len(), seqs.as_ptr(), min_len.as_ptr(), seqs.len(), regions, lanes, threshold, &mut raw,
            ))?;
        }
        Ok(Matcher { raw, lanes })
    }

    /// The hashes every lane has received since the last feed: one slice per lane, an empty one for nothing.
    pub fn feed(&mut self, items: &[&[u32]]) -> Result<()> {
        assert_eq!(items.len(), self.lanes, "one slice per lane");
        let ptrs: Vec<*const u32> = items.iter().map(|s| s.as_ptr()).collect();
        let lens: Vec<usize> = items.iter().map(|s| s.len()).collect();
        unsafe { check(ffi::needle_hip_matcher_feed(self.raw, ptrs.as_ptr(), lens.as_ptr())) }
    }

    /// Takes, lane by lane, the feeder's ready items this matcher has not yet taken, and finishes the lanes it has finished.
    pub fn feed_from_feeder(&mut self, feeder: &mut Feeder) -> Result<()> {
        unsafe { check(ffi::needle_hip_matcher_feed_from_feeder(self.raw, feeder.raw)) }
    }

    /// `None`: every unfinished lane.
    pub fn finish(&mut self, lanes: Option<&[usize]>) -> Result<()> {
        let (p, k) = lanes.map_or((ptr::null(), 0), |l| (l.as_ptr(), l.len()));
        unsafe { check(ffi::needle_hip_matcher_finish(self.raw, p, k)) }
    }

    /// The lanes start new streams (`None`: every lane).
    pub fn reset(&mut self, lanes: Option<&[usize]>) -> Result<()> {
        let (p, k) = lanes.map_or((ptr::null(), 0), |l| (l.as_ptr(), l.len()));
        unsafe { check(ffi::needle_hip_matcher_reset(self.raw, p, k)) }
    }

    /// `(runs reported, items fed, finished)` of a lane.
    pub fn ready(&mut self, lane: usize) -> Result<(usize, u64, bool)> {
        let (mut runs, mut fed, mut finished) = (0usize, 0u64, false);
        unsafe { check(ffi::needle_hip_matcher_ready(self.raw, lane, &mut runs, &mut fed, &mut finished))? };
        Ok((runs, fed, finished))
    }

    /// Runs `[first, first + count)` of a lane, in the order they were reported; `problem` is the source's index.
    pub fn runs(&mut self, lane: usize, first: usize, count: usize) -> Result<Vec<ffi::NeedleHipRun>> {
        let mut out = vec![ffi::NeedleHipRun::default(); count];
        unsafe { check(ffi::needle_hip_matcher_runs(self.raw, lane, first, count, out.as_mut_ptr()))? };
        Ok(out)
    }

    /// The runs still open at the last column fed whose length is already `>= min_len` (simhash fields zero).
    pub fn open(&mut self, lane: usize) -> Result<Vec<ffi::NeedleHipRun>> {
        let (mut runs, mut n) = (ptr::null_mut(), 0usize);
        unsafe {
            check(ffi::needle_hip_matcher_open(self.raw, lane, &mut runs, &mut n))?;
            let out = std::slice::from_raw_parts(runs as *const ffi::NeedleHipRun, n).to_vec();
            ffi::needle_hip_host_free(runs as *mut std::os::raw::c_void);
            Ok(out)
        }
    }

    /// `(feeds, kernel launches, cells evaluated, bytes of state on the device)`.
    pub fn stats(&self) -> Result<(u64, u64, u64, u64)> {
        let mut stats = [0u64; 4];
        unsafe { check(ffi::needle_hip_matcher_stats(self.raw, stats.as_mut_ptr()))? };
        Ok((stats[0], stats[1], stats[2], stats[3]))
    }
}

impl Drop for Matcher {
    fn drop(&mut self) {
        unsafe { ffi::needle_hip_matcher_free(self.raw) };
    }
}

/// Streaming all-pairs comparator (`needle_hip_crossmatcher_*`): the lanes are the videos of a season, matched against each
/// other as their hashes arrive.  `problem` of a run is the pair's index in the comparator's i-major order, so the list goes
/// straight into the host epilogue.  After every lane is finished the runs equal the one-shot scan's over all pairs.
pub struct CrossMatcher {
    raw: *mut ffi::NeedleHipCrossMatcher,
    lanes: usize,
}

unsafe impl Send for CrossMatcher {}

impl CrossMatcher {
    /// `lanes` in 2..=256, every lane holds at most `max_items`.  Fails without a HIP device: the state is allocated here.
    pub fn new(lanes: usize, max_items: usize, min_len: u32, threshold: u32) -> Result<Self> {
        let mut raw = ptr::null_mut();
        unsafe { check(ffi::needle_hip_crossmatcher_new(lanes, max_items, min_len, threshold, &mut raw))? };
        Ok(CrossMatcher { raw, lanes })
    }

    /// Openings and endings in one object: `videos * max_items.len()` lanes, lane = video * regions + region, matched within a
    /// region only; `max_items` and `min_len` hold one entry per region (1 or 2).  `problem` of a run is pair * regions + region.
    pub fn with_regions(videos: usize, max_items: &[usize], min_len: &[u32], threshold: u32) -> Result<Self> {
        assert_eq!(max_items.len(), min_len.len(), "one max_items and one min_len per region");
        let regions = max_items.len();
        let mut raw = ptr::null_mut();
        unsafe {
            check(ffi::needle_hip_crossmatcher_new_regions(videos, regions, max_items.as_ptr(), min_len.as_ptr(), threshold, &mut raw))?
        };
        Ok(CrossMatcher { raw, lanes: videos * regions })
    }

    /// A new season joins a library: `resident` holds the hashes of the K known videos in row order (video k, region r at
    /// `k * regions + r`, regions = `max_items.len()`), uploaded here; `videos` arriving videos follow them in the video list
    /// and own the `videos * regions` lanes.  Only pairs with an arriving end are searched; `problem` of a run numbers the
    /// pairs over all K + `videos` videos, so the list goes into `results_from_runs` with `first_video = K`.
    pub fn with_resident(resident: &[&[u32]], videos: usize, max_items: &[usize], min_len: &[u32], threshold: u32) -> Result<Self> {
        assert_eq!(max_items.len(), min_len.len(), "one max_items and one min_len per region");
        let regions = max_items.len();
        assert!(regions > 0 && resident.len() % regions == 0, "one resident row per video and region");
        let mut arena: Vec<u32> = Vec::new();
        let mut seqs = Vec::with_capacity(resident.len());
        for hashes in resident {
            seqs.push(ffi::NeedleHipSeq { offset: arena.len() as u32, len: hashes.len() as u32 });
            arena.extend_from_slice(hashes);
        }
        let mut raw = ptr::null_mut();
        unsafe {
            check(ffi::needle_hip_crossmatcher_new_resident(
                arena.as_ptr(),
                arena.len(),
                seqs.as_ptr(),
                seqs.len() / regions,
                videos,
                regions,
                max_items.as_ptr(),
                min_len.as_ptr(),
                threshold,
                &mut raw,
            ))?
        };
        Ok(CrossMatcher { raw, lanes: videos * regions })
    }

    /// Groups of videos: `groups[t]` is the label of arriving video t, `resident_groups[k]` that of resident k, whose rows are
    /// `resident` as in `with_resident` (both may be empty).  Only same-label pairs with an arriving end are live; `problem`
    /// of a run is (the grouped pair id over all K + N labels) * regions + region, the numbering `group_pairs` decodes.
    pub fn with_groups(
        resident: &[&[u32]],
        resident_groups: &[u32],
        groups: &[u32],
        max_items: &[usize],
        min_len: &[u32],
        threshold: u32,
    ) -> Result<Self> {
        assert_eq!(max_items.len(), min_len.len(), "one max_items and one min_len per region");
        let regions = max_items.len();
        assert!(regions > 0 && resident.len() == resident_groups.len() * regions, "one resident row per video and region");
        let mut arena: Vec<u32> = Vec::new();
        let mut seqs = Vec::with_capacity(resident.len());
        for hashes in resident {
            seqs.push(ffi::NeedleHipSeq { offset: arena.len() as u32, len: hashes.len() as u32 });
            arena.extend_from_slice(hashes);
        }
        let mut raw = ptr::null_mut();
        unsafe {
            check(ffi::needle_hip_crossmatcher_new_grouped(
                arena.as_ptr(),
                arena.len(),
                seqs.as_ptr(),
                resident_groups.len(),
                resident_groups.as_ptr(),
                groups.len(),
                groups.as_ptr(),
                regions,
                max_items.as_ptr(),
                min_len.as_ptr(),
                threshold,
                &mut raw,
            ))?
        };
        Ok(CrossMatcher { raw, lanes: groups.len() * regions })
    }

    /// The labels of all K + N videos of a grouped object, residents first; an error for an object without groups.
    pub fn groups(&self) -> Result<Vec<u32>> {
        let (videos, _) = self.shape()?;
        let mut labels = vec![0u32; self.resident()? + videos];
        unsafe { check(ffi::needle_hip_crossmatcher_groups(self.raw, labels.as_mut_ptr(), labels.len()))? };
        Ok(labels)
    }

    /// Bytes of frontiers and hashes a grouped object allocates (resident rows of these lengths, row order); 0 where
    /// creation would refuse.
    pub fn state_bytes_grouped(resident_len: &[u32], resident_groups: &[u32], groups: &[u32], max_items: &[usize]) -> usize {
        let seqs: Vec<ffi::NeedleHipSeq> = resident_len.iter().map(|&len| ffi::NeedleHipSeq { offset: 0, len }).collect();
        unsafe {
            ffi::needle_hip_crossmatcher_state_bytes_grouped(
                seqs.as_ptr(),
                resident_groups.len(),
                resident_groups.as_ptr(),
                groups.len(),
                groups.as_ptr(),
                max_items.len(),
                max_items.as_ptr(),
            )
        }
    }

    /// The known videos the object was created with (0 without `with_resident`).
    pub fn resident(&self) -> Result<usize> {
        let mut k = 0usize;
        unsafe { check(ffi::needle_hip_crossmatcher_resident(self.raw, &mut k))? };
        Ok(k)
    }

    /// Bytes of device state of a matcher with resident rows of these lengths (row order); 0 where an argument is out of range.
    pub fn state_bytes_resident(resident_len: &[u32], videos: usize, max_items: &[usize]) -> usize {
        let regions = max_items.len().max(1);
        let seqs: Vec<ffi::NeedleHipSeq> = resident_len.iter().map(|&len| ffi::NeedleHipSeq { offset: 0, len }).collect();
        unsafe { ffi::needle_hip_crossmatcher_state_bytes_resident(seqs.as_ptr(), seqs.len() / regions, videos, max_items.len(), max_items.as_ptr()) }
    }

    /// `(videos, regions)`: the arriving videos; the object has `videos * regions` lanes.
    pub fn shape(&self) -> Result<(usize, usize)> {
        let (mut videos, mut regions) = (0usize, 0usize);
        unsafe { check(ffi::needle_hip_crossmatcher_shape(self.raw, &mut videos, &mut regions))? };
        Ok((videos, regions))
    }

    /// Bytes of device state such a matcher allocates (pure host arithmetic).
    pub fn state_bytes(lanes: usize, max_items: usize) -> usize {
        unsafe { ffi::needle_hip_crossmatcher_state_bytes(lanes, max_items) }
    }

    /// The same for one capacity per region; 0 where an argument is out of range.
    pub fn state_bytes_regions(videos: usize, max_items: &[usize]) -> usize {
        unsafe { ffi::needle_hip_crossmatcher_state_bytes_regions(videos, max_items.len(), max_items.as_ptr()) }
    }

    /// The hashes every lane has received since the last feed: one slice per lane, an empty one for nothing.
    pub fn feed(&mut self, items: &[&[u32]]) -> Result<()> {
        assert_eq!(items.len(), self.lanes, "one slice per lane");
        let ptrs: Vec<*const u32> = items.iter().map(|s| s.as_ptr()).collect();
        let lens: Vec<usize> = items.iter().map(|s| s.len()).collect();
        unsafe { check(ffi::needle_hip_crossmatcher_feed(self.raw, ptrs.as_ptr(), lens.as_ptr())) }
    }

    /// Takes, lane by lane, the feeder's ready items this matcher has not yet taken, and finishes the lanes it has finished.
    pub fn feed_from_feeder(&mut self, feeder: &mut Feeder) -> Result<()> {
        unsafe { check(ffi::needle_hip_crossmatcher_feed_from_feeder(self.raw, feeder.raw)) }
    }

    /// `None`: every unfinished lane.
    pub fn finish(&mut self, lanes: Option<&[usize]>) -> Result<()> {
        let (p, k) = lanes.map_or((ptr::null(), 0), |l| (l.as_ptr(), l.len()));
        unsafe { check(ffi::needle_hip_crossmatcher_finish(self.raw, p, k)) }
    }

    /// `(runs reported, every lane finished)`.
    pub fn ready(&mut self) -> Result<(usize, bool)> {
        let (mut runs, mut complete) = (0usize, false);
        unsafe { check(ffi::needle_hip_crossmatcher_ready(self.raw, &mut runs, &mut complete))? };
        Ok((runs, complete))
    }

    /// `(items fed, finished)` of a lane.
    pub fn lane(&mut self, lane: usize) -> Result<(u64, bool)> {
        let (mut fed, mut finished) = (0u64, false);
        unsafe { check(ffi::needle_hip_crossmatcher_lane(self.raw, lane, &mut fed, &mut finished))? };
        Ok((fed, finished))
    }

    /// Runs `[first, first + count)` of the list, in the order they were reported.
    pub fn runs(&mut self, first: usize, count: usize) -> Result<Vec<ffi::NeedleHipRun>> {
        let mut out = vec![ffi::NeedleHipRun::default(); count];
        unsafe { check(ffi::needle_hip_crossmatcher_runs(self.raw, first, count, out.as_mut_ptr()))? };
        Ok(out)
    }

    /// `(feeds, kernel launches, cells evaluated, bytes of state on the device)`.
    pub fn stats(&self) -> Result<(u64, u64, u64, u64)> {
        let mut stats = [0u64; 4];
        unsafe { check(ffi::needle_hip_crossmatcher_stats(self.raw, stats.as_mut_ptr()))? };
        Ok((stats[0], stats[1], stats[2], stats[3]))
    }
}

impl Drop for CrossMatcher {
    fn drop(&mut self) {
        unsafe { ffi::needle_hip_crossmatcher_free(self.raw) };
    }
}

/// An incremental search index (include/needle_hip.h "Incremental index"): `results()` equals
/// `Comparator::run_with_frame_hashes` over the index's current list of videos (one slot per video, `None` where that call
/// pushes no result); `add` searches only the pairs it adds, `remove` none and `replace` those of the videos replaced.  The comparator's parameters are copied at
/// creation.  One GPU: the device current at creation.
pub struct Index {
    raw: *mut ffi::NeedleHipIndex,
}

unsafe impl Send for Index {}

impl Index {
    pub fn new<P: AsRef<Path>>(comparator: &Comparator<P>) -> Result<Self> {
        let handle = comparator.handle()?;
        let mut raw = ptr::null_mut();
        let status = unsafe { check(ffi::needle_hip_index_new(handle, &mut raw)) };
        unsafe { ffi::needle_audio_comparator_free(handle) };
        status?;
        Ok(Index { raw })
    }

    /// Appends the videos (their hashes are copied).  On error the index is as it was before the call.
    pub fn add(&mut self, frame_hashes: &[&FrameHashes]) -> Result<()> {
        let raw: Vec<*const ffi::FrameHashes> = frame_hashes.iter().map(|f| f.raw as *const _).collect();
        unsafe { check(ffi::needle_hip_index_add(self.raw, raw.as_ptr(), raw.len())) }
    }

    /// A grouped index (include/needle_hip.h "A grouped index"): a library of many seasons.  Videos are added with a label
    /// each (`add_grouped`), only pairs inside a season are searched, and `results()` equals
    /// `Comparator::run_with_frame_hashes_grouped` over the current list.
    pub fn new_grouped<P: AsRef<Path>>(comparator: &Comparator<P>) -> Result<Self> {
        let handle = comparator.handle()?;
        let mut raw = ptr::null_mut();
        let status = unsafe { check(ffi::needle_hip_index_new_grouped(handle, &mut raw)) };
        unsafe { ffi::needle_audio_comparator_free(handle) };
        status?;
        Ok(Index { raw })
    }

    /// Appends the videos to a grouped index, `groups[i]` the label of `frame_hashes[i]` (any values: they are only compared).
    pub fn add_grouped(&mut self, frame_hashes: &[&FrameHashes], groups: &[u32]) -> Result<()> {
        if groups.len() != frame_hashes.len() {
            return Err(Error {
                code: ffi::NeedleError::InvalidArgument,
                message: "index add_grouped: one group label per video".into(),
            });
        }
        let raw: Vec<*const ffi::FrameHashes> = frame_hashes.iter().map(|f| f.raw as *const _).collect();
        unsafe { check(ffi::needle_hip_index_add_grouped(self.raw, raw.as_ptr(), groups.as_ptr(), raw.len())) }
    }

    /// The current list's labels, one per video (a grouped index; an error on a plain one).
    pub fn groups(&self) -> Result<Vec<u32>> {
        let mut labels = vec![0u32; self.len()];
        unsafe { check(ffi::needle_hip_index_groups(self.raw, labels.as_mut_ptr(), labels.len()))? };
        Ok(labels)
    }

    /// Removes the videos at these distinct positions; the others keep their order.  No pair is searched.  On error the
    /// index is as it was before the call.
    pub fn remove(&mut self, positions: &[usize]) -> Result<()> {
        unsafe { check(ffi::needle_hip_index_remove(self.raw, positions.as_ptr(), positions.len())) }
    }

    /// Replaces the video at `positions[i]` with `frame_hashes[i]`, in place; only the pairs of those videos are searched.
    /// On error the index is as it was before the call.
    pub fn replace(&mut self, positions: &[usize], frame_hashes: &[&FrameHashes]) -> Result<()> {
        if positions.len() != frame_hashes.len() {
            return Err(Error {
                code: ffi::NeedleError::InvalidArgument,
                message: "index replace: one FrameHashes per position".into(),
            });
        }
        let raw: Vec<*const ffi::FrameHashes> = frame_hashes.iter().map(|f| f.raw as *const _).collect();
        unsafe { check(ffi::needle_hip_index_replace(self.raw, positions.as_ptr(), raw.as_ptr(), raw.len())) }
    }

    /// [heap entries held, entry slots in use, hashes in the device arena, timestamps in the device table].
    pub fn store_sizes(&self) -> Result<[u64; 4]> {
        let mut sizes = [0u64; 4];
        unsafe { check(ffi::needle_hip_index_store_sizes(self.raw, sizes.as_mut_ptr()))? };
        Ok(sizes)
    }

    pub fn len(&self) -> usize {
        unsafe { ffi::needle_hip_index_len(self.raw) }
    }

    pub fn is_empty(&self) -> bool {
        self.len() == 0
    }

    pub fn results(&self) -> Result<Vec<Option<SearchResult>>> {
        let mut results = vec![ffi::NeedleHipSearchResult::default(); self.len()];
        unsafe { check(ffi::needle_hip_index_results(self.raw, results.as_mut_ptr(), results.len()))? };
        let span = |a: u64, b: u64| (Duration::from_nanos(a), Duration::from_nanos(b));
        Ok(results
            .into_iter()
            .map(|r| {
                r.has_result.then(|| SearchResult {
                    opening: r.has_opening.then(|| span(r.opening_start_ns, r.opening_end_ns)),
                    ending: r.has_ending.then(|| span(r.ending_start_ns, r.ending_end_ns)),
                })
            })
            .collect())
    }

    /// Why every video got its result (`needle_hip_index_evidence`): one record per video, computed on the device from the
    /// committed store when asked; `partner` is a current position.  The index is not changed.
    pub fn evidence(&self) -> Result<Vec<SearchEvidence>> {
        let mut evidence = vec![ffi::NeedleHipSearchEvidence::default(); self.len()];
        unsafe { check(ffi::needle_hip_index_evidence(self.raw, evidence.as_mut_ptr(), evidence.len()))? };
        Ok(evidence.into_iter().map(SearchEvidence::from).collect())
    }

    /// (total, last): video pairs that entered the index over its life and by the last `add`.
    pub fn pairs_searched(&self) -> Result<(u64, u64)> {
        let (mut total, mut last) = (0u64, 0u64);
        unsafe { check(ffi::needle_hip_index_pairs_searched(self.raw, &mut total, &mut last))? };
        Ok((total, last))
    }

    /// (total, last): video pairs handed to the one-shot scan over the index's life and by the last operation (0 after
    /// `add_matched`).
    pub fn pairs_scanned(&self) -> Result<(u64, u64)> {
        let (mut total, mut last) = (0u64, 0u64);
        unsafe { check(ffi::needle_hip_index_pairs_scanned(self.raw, &mut total, &mut last))? };
        Ok((total, last))
    }

    /// A cross-matcher whose resident videos are this index's, in its order (their rows are copied from the index's device
    /// arena), with `videos` arriving ones; regions and threshold are the index's, `max_items` and `min_len` hold one entry
    /// per region.  Feed it as the season decodes, then hand it to `add_matched`.
    pub fn crossmatcher(&mut self, videos: usize, max_items: &[usize], min_len: &[u32]) -> Result<CrossMatcher> {
        assert_eq!(max_items.len(), min_len.len(), "one max_items and one min_len per region");
        let mut raw = ptr::null_mut();
        unsafe { check(ffi::needle_hip_index_crossmatcher_new(self.raw, videos, max_items.as_ptr(), min_len.as_ptr(), &mut raw))? };
        Ok(CrossMatcher { raw, lanes: videos * max_items.len() })
    }

    /// Appends the arriving videos of `matcher` (complete, made by `crossmatcher` since the index last changed) with the runs
    /// it holds in place of a scan: afterwards the index is what `add(frame_hashes)` leaves, and no pair was searched twice.
    /// On error the index is as it was before the call.
    pub fn add_matched(&mut self, matcher: &mut CrossMatcher, frame_hashes: &[&FrameHashes]) -> Result<()> {
        let raw: Vec<*const ffi::FrameHashes> = frame_hashes.iter().map(|f| f.raw as *const _).collect();
        unsafe { check(ffi::needle_hip_index_add_matched(self.raw, matcher.raw, raw.as_ptr(), raw.len())) }
    }

    /// `crossmatcher` for a grouped index: the residents carry the index's labels, `groups[t]` is the label of arriving video
    /// t, and only same-label pairs are live.  Hand it to `add_matched_grouped`.
    pub fn crossmatcher_grouped(&mut self, groups: &[u32], max_items: &[usize], min_len: &[u32]) -> Result<CrossMatcher> {
        assert_eq!(max_items.len(), min_len.len(), "one max_items and one min_len per region");
        let mut raw = ptr::null_mut();
        unsafe {
            check(ffi::needle_hip_index_crossmatcher_new_grouped(
                self.raw,
                groups.len(),
                groups.as_ptr(),
                max_items.as_ptr(),
                min_len.as_ptr(),
                &mut raw,
            ))?
        };
        Ok(CrossMatcher { raw, lanes: groups.len() * max_items.len() })
    }

    /// Appends the arriving videos of a grouped `matcher` under its labels, with its runs in place of a scan: afterwards the
    /// index is what `add_grouped` leaves.  On error the index is as it was before the call.
    pub fn add_matched_grouped(&mut self, matcher: &mut CrossMatcher, frame_hashes: &[&FrameHashes]) -> Result<()> {
        let raw: Vec<*const ffi::FrameHashes> = frame_hashes.iter().map(|f| f.raw as *const _).collect();
        unsafe { check(ffi::needle_hip_index_add_matched_grouped(self.raw, matcher.raw, raw.as_ptr(), raw.len())) }
    }
}

impl Index {
    /// A matcher whose sources are this index's rows (gathered from the index's device arena), with `videos * regions`
    /// lanes; `regions` is the index's (2 with endings).  The resident x arriving half of a streamed season at any library
    /// size: feed it and a `CrossMatcher::with_regions` over the same videos, then hand both to `add_streamed`.
    pub fn matcher(&mut self, videos: usize, regions: usize) -> Result<Matcher> {
        let mut raw = ptr::null_mut();
        unsafe { check(ffi::needle_hip_index_matcher_new(self.raw, videos, &mut raw))? };
        Ok(Matcher { raw, lanes: videos * regions })
    }

    /// Appends the arriving videos with the runs of `matcher` (made by `matcher` since the index last changed) for the
    /// resident x arriving pairs and those of `crossmatcher` (no residents; `None` with one video) for the arriving pairs.
    /// Afterwards the index is what `add(frame_hashes)` leaves; on error it is as it was before the call.
    pub fn add_streamed(&mut self, matcher: &mut Matcher, crossmatcher: Option<&mut CrossMatcher>, frame_hashes: &[&FrameHashes]) -> Result<()> {
        let raw: Vec<*const ffi::FrameHashes> = frame_hashes.iter().map(|f| f.raw as *const _).collect();
        let cross = crossmatcher.map_or(ptr::null_mut(), |c| c.raw);
        unsafe { check(ffi::needle_hip_index_add_streamed(self.raw, matcher.raw, cross, raw.as_ptr(), raw.len())) }
    }
}

impl Drop for Index {
    fn drop(&mut self) {
        unsafe { ffi::needle_hip_index_free(self.raw) };
    }
}

fn optional_result(r: ffi::NeedleHipSearchResult) -> Option<SearchResult> {
    let span = |a: u64, b: u64| (Duration::from_nanos(a), Duration::from_nanos(b));
    r.has_result.then(|| SearchResult {
        opening: r.has_opening.then(|| span(r.opening_start_ns, r.opening_end_ns)),
        ending: r.has_ending.then(|| span(r.ending_start_ns, r.ending_end_ns)),
    })
}

/// The pairs a grouped search compares, in the order of their ids (`needle_hip_group_pairs`): `groups` has a label per
/// video, only videos of equal label form a pair, and `NeedleHipRun.problem / regions` of a grouped run list indexes
/// this list.
pub fn group_pairs(groups: &[u32]) -> Result<Vec<(u32, u32)>> {
    let mut count = 0u64;
    unsafe { check(ffi::needle_hip_group_pairs(groups.as_ptr(), groups.len(), std::ptr::null_mut(), 0, &mut count))? };
    let mut flat = vec![0u32; 2 * count as usize];
    unsafe { check(ffi::needle_hip_group_pairs(groups.as_ptr(), groups.len(), flat.as_mut_ptr(), count as usize, &mut count))? };
    Ok(flat.chunks_exact(2).map(|p| (p[0], p[1])).collect())
}

/// A copy of `n` values the library malloc'd at `p`, which is freed.
unsafe fn take_host<T: Copy>(p: *mut T, n: usize) -> Vec<T> {
    let out = if n == 0 { Vec::new() } else { std::slice::from_raw_parts(p as *const T, n).to_vec() };
    ffi::needle_hip_host_free(p as *mut std::os::raw::c_void);
    out
}

/// The most bytes a fingerprint of `items` items compresses to.
pub fn fingerprint_compressed_bound(items: usize) -> usize {
    unsafe { ffi::needle_hip_fingerprint_compressed_bound(items) }
}

/// `(items of a compress tile, 3-bit symbols of a decompress tile)` of the device codec.
pub fn fingerprint_codec_tiles() -> Result<(usize, usize)> {
    let (mut t, mut d) = (0usize, 0usize);
    unsafe { check(ffi::needle_hip_fingerprint_codec_tiles(&mut t, &mut d))? };
    Ok((t, d))
}

/// Each fingerprint in chromaprint's compressed form (`FingerprintCompressor`), on the device, all in one call.
pub fn compress_fingerprints(fingerprints: &[&[u32]], algorithm: i32) -> Result<Vec<Vec<u8>>> {
    let items: Vec<u32> = fingerprints.iter().flat_map(|f| f.iter().copied()).collect();
    let mut off = vec![0u64; fingerprints.len() + 1];
    for (b, f) in fingerprints.iter().enumerate() {
        off[b + 1] = off[b] + f.len() as u64;
    }
    let mut blob_off = vec![0u64; fingerprints.len() + 1];
    let mut blobs = ptr::null_mut();
    unsafe {
        check(ffi::needle_hip_fingerprint_compress_host(items.as_ptr(), off.as_ptr(), fingerprints.len(), algorithm, &mut blobs, blob_off.as_mut_ptr()))?;
        let data = take_host(blobs, blob_off[fingerprints.len()] as usize);
        Ok(blob_off.windows(2).map(|w| data[w[0] as usize..w[1] as usize].to_vec()).collect())
    }
}

/// One decompressed fingerprint: `status` 0 ok, 1 shorter than a header, 2 the normal stream ends early, 3 the exceptional
/// stream ends early, 4 a bit position above 32; the items of a refused blob are empty.
pub struct Decompressed {
    pub items: Vec<u32>,
    pub algorithm: i32,
    pub status: i32,
}

/// Compressed fingerprints back to items (`FingerprintDecompressor`), on the device, all in one call.
pub fn decompress_fingerprints(blobs: &[&[u8]]) -> Result<Vec<Decompressed>> {
    let data: Vec<u8> = blobs.iter().flat_map(|b| b.iter().copied()).collect();
    let mut off = vec![0u64; blobs.len() + 1];
    for (b, blob) in blobs.iter().enumerate() {
        off[b + 1] = off[b] + blob.len() as u64;
    }
    let mut item_off = vec![0u64; blobs.len() + 1];
    let (mut algorithms, mut status) = (vec![0i32; blobs.len()], vec![0i32; blobs.len()]);
    let mut items = ptr::null_mut();
    unsafe {
        check(ffi::needle_hip_fingerprint_decompress_host(
            data.as_ptr(),
            off.as_ptr(),
            blobs.len(),
            &mut items,
            item_off.as_mut_ptr(),
            algorithms.as_mut_ptr(),
            status.as_mut_ptr(),
        ))?;
        let flat = take_host(items, item_off[blobs.len()] as usize);
        Ok((0..blobs.len())
            .map(|b| Decompressed { items: flat[item_off[b] as usize..item_off[b + 1] as usize].to_vec(), algorithm: algorithms[b], status: status[b] })
            .collect())
    }
}

/// base64 with the URL-safe alphabet and no padding: the text form of a compressed fingerprint.
pub fn base64_encode(data: &[u8]) -> Result<String> {
    let (mut text, mut size) = (ptr::null_mut(), 0usize);
    unsafe {
        check(ffi::needle_hip_fingerprint_base64_encode(data.as_ptr(), data.len(), &mut text, &mut size))?;
        Ok(String::from_utf8_lossy(&take_host(text as *mut u8, size)).into_owned())
    }
}

/// Refuses characters outside the alphabet and a length of 1 mod 4.
pub fn base64_decode(text: &str) -> Result<Vec<u8>> {
    let (mut data, mut size) = (ptr::null_mut(), 0usize);
    unsafe {
        check(ffi::needle_hip_fingerprint_base64_decode(text.as_ptr() as *const std::os::raw::c_char, text.len(), &mut data, &mut size))?;
        Ok(take_host(data, size))
    }
}

/// chromaprint's 32-bit simhash of a fingerprint; 0 for an empty one.
pub fn fingerprint_simhash(items: &[u32]) -> Result<u32> {
    let mut hash = 0u32;
    unsafe { check(ffi::needle_hip_fingerprint_simhash(items.as_ptr(), items.len(), &mut hash))? };
    Ok(hash)
}

/// Number of HIP devices the library sees (0 on a host without a GPU: every compute call then fails loudly).
pub fn device_count() -> Result<i32> {
    let mut n = 0;
    unsafe { check(ffi::needle_hip_device_count(&mut n))? };
    Ok(n)
}

/// Interleaved channels the analyze paths accept (`NEEDLE_HIP_MAX_CHANNELS`): 1..=8.
pub const MAX_CHANNELS: i32 = 8;

/// The device down-mix on its own: each stream of interleaved s16 with `channels` (1..=MAX_CHANNELS) channels to mono,
/// `(sum of a frame) / channels` with C truncation, a trailing partial frame dropped.  Every analyze path applies it to
/// 3-8 channel input; this form is for callers that want the mono signal itself.
pub fn downmix(pcm: &[&[i16]], channels: i32) -> Result<Vec<Vec<i16>>> {
    let per = channels.max(1) as usize;
    let mut out: Vec<Vec<i16>> = pcm.iter().map(|s| vec![0i16; s.len() / per]).collect();
    let ptrs: Vec<*const i16> = pcm.iter().map(|s| s.as_ptr()).collect();
    let lens: Vec<usize> = pcm.iter().map(|s| s.len()).collect();
    let optrs: Vec<*mut i16> = out.iter_mut().map(|o| o.as_mut_ptr()).collect();
    unsafe {
        check(ffi::needle_hip_downmix_host(ptrs.as_ptr(), lens.as_ptr(), pcm.len(), channels, optrs.as_ptr()))?;
    }
    Ok(out)
}

/// `NeedleHipSampleFormat`: how a decoder hands samples over (FFmpeg's `AVSampleFormat` numbering, so `frame.format` can
/// be passed through).  The planar forms take one slice per channel.
#[repr(i32)]
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub enum SampleFormat {
    U8 = 0,
    S16 = 1,
    S32 = 2,
    F32 = 3,
    F64 = 4,
    U8P = 5,
    S16P = 6,
    S32P = 7,
    F32P = 8,
    F64P = 9,
}

/// A sample type the device converts to s16 (`needle_hip.h`, "sample formats"): u8 `(x - 128) << 8`, i32 `x >> 16`,
/// f32 / f64 `rint(x * 32768)` with NaN -> 0 and clipping.
pub trait Sample: Copy {
    const INTERLEAVED: SampleFormat;
    const PLANAR: SampleFormat;
}
impl Sample for u8 {
    const INTERLEAVED: SampleFormat = SampleFormat::U8;
    const PLANAR: SampleFormat = SampleFormat::U8P;
}
impl Sample for i16 {
    const INTERLEAVED: SampleFormat = SampleFormat::S16;
    const PLANAR: SampleFormat = SampleFormat::S16P;
}
impl Sample for i32 {
    const INTERLEAVED: SampleFormat = SampleFormat::S32;
    const PLANAR: SampleFormat = SampleFormat::S32P;
}
impl Sample for f32 {
    const INTERLEAVED: SampleFormat = SampleFormat::F32;
    const PLANAR: SampleFormat = SampleFormat::F32P;
}
impl Sample for f64 {
    const INTERLEAVED: SampleFormat = SampleFormat::F64;
    const PLANAR: SampleFormat = SampleFormat::F64P;
}

/// The device sample-format conversion on its own (`needle_hip_convert_host`): every stream to interleaved
/// `channels`-channel s16, not down-mixed.  `planar`: `pcm` holds `channels` slices (planes) per stream, one after the
/// other, each of the stream's frame count; otherwise one interleaved slice per stream.
pub fn convert<T: Sample>(pcm: &[&[T]], channels: i32, planar: bool) -> Result<Vec<Vec<i16>>> {
    let per = channels.max(1) as usize;
    let planes = if planar { per } else { 1 };
    assert!(pcm.len() % planes == 0, "one slice per plane of every stream");
    let lens: Vec<usize> = pcm.chunks(planes).map(|s| s.iter().map(|p| p.len()).sum()).collect();
    let mut out: Vec<Vec<i16>> = lens.iter().map(|n| vec![0i16; n / per * per]).collect();
    let ptrs: Vec<*const std::os::raw::c_void> = pcm.iter().map(|s| s.as_ptr() as *const _).collect();
    let optrs: Vec<*mut i16> = out.iter_mut().map(|o| o.as_mut_ptr()).collect();
    let format = if planar { T::PLANAR } else { T::INTERLEAVED };
    unsafe {
        check(ffi::needle_hip_convert_host(ptrs.as_ptr(), lens.as_ptr(), lens.len(), channels, format as i32, optrs.as_ptr()))?;
    }
    Ok(out)
}

/// A channel mix (`needle_hip.h`, "Channel mixes"): the layout-aware fold-down to stereo, then mono.
pub use ffi::NeedleHipChannelMix as ChannelMix;

/// `needle_hip_channel_mix_default`: the default mix of a WAVEFORMATEXTENSIBLE / FFmpeg channel mask (host arithmetic).
pub fn channel_mix_default(channel_mask: u32) -> Result<ChannelMix> {
    let mut mix = ChannelMix::default();
    unsafe { check(ffi::needle_hip_channel_mix_default(channel_mask, &mut mix))? };
    Ok(mix)
}

/// `needle_hip_rematrix_host`: `convert_mono` with a channel mix per stream (channels 0: the plain average of that
/// stream), one launch of the rematrix kernel whatever the mixture.
pub fn rematrix(pcm: &[&[&[u8]]], formats: &[LaneFormat], mixes: &[ChannelMix]) -> Result<Vec<Vec<i16>>> {
    assert!(pcm.len() == formats.len() && pcm.len() == mixes.len(), "one format and one mix per stream");
    let (mut ptrs, mut lens) = (Vec::new(), Vec::with_capacity(pcm.len()));
    for (planes, f) in pcm.iter().zip(formats) {
        assert_eq!(planes.len(), format_planes(f), "one slice per plane of the stream");
        let width = [1usize, 2, 4, 4, 8][(f.format % 5) as usize];
        ptrs.extend(planes.iter().map(|s| s.as_ptr() as *const std::os::raw::c_void));
        lens.push(planes.iter().map(|p| p.len() / width).sum::<usize>());
    }
    let mut out: Vec<Vec<i16>> = lens.iter().zip(formats).map(|(n, f)| vec![0i16; n / f.channels.max(1) as usize]).collect();
    let optrs: Vec<*mut i16> = out.iter_mut().map(|o| o.as_mut_ptr()).collect();
    unsafe {
        check(ffi::needle_hip_rematrix_host(ptrs.as_ptr(), lens.as_ptr(), formats.as_ptr(), mixes.as_ptr(), formats.len(), optrs.as_ptr()))?;
    }
    Ok(out)
}

/// `needle_hip_convert_mono_host`: streams that each have a format of their own -> mono s16 (`convert`, then `downmix`, in
/// one kernel whatever the mixture).  Per stream the raw bytes of its planes, as in `Feeder::feed_lanes`; the formats'
/// sample rates are not looked at.
pub fn convert_mono(pcm: &[&[&[u8]]], formats: &[LaneFormat]) -> Result<Vec<Vec<i16>>> {
    assert_eq!(pcm.len(), formats.len(), "one format per stream");
    let (mut ptrs, mut lens) = (Vec::new(), Vec::with_capacity(pcm.len()));
    for (planes, f) in pcm.iter().zip(formats) {
        assert_eq!(planes.len(), format_planes(f), "one slice per plane of the stream");
        let width = [1usize, 2, 4, 4, 8][(f.format % 5) as usize];
        ptrs.extend(planes.iter().map(|s| s.as_ptr() as *const std::os::raw::c_void));
        lens.push(planes.iter().map(|p| p.len() / width).sum::<usize>());
    }
    let mut out: Vec<Vec<i16>> = lens.iter().zip(formats).map(|(n, f)| vec![0i16; n / f.channels.max(1) as usize]).collect();
    let optrs: Vec<*mut i16> = out.iter_mut().map(|o| o.as_mut_ptr()).collect();
    unsafe {
        check(ffi::needle_hip_convert_mono_host(ptrs.as_ptr(), lens.as_ptr(), formats.as_ptr(), formats.len(), optrs.as_ptr()))?;
    }
    Ok(out)
}

/// Frame-hash file next to a video: `Path::with_extension("needle.dat")` (data.rs:8-13,117-119).
pub fn frame_hash_path(video: impl AsRef<Path>) -> PathBuf {
    video.as_ref().with_extension("needle.dat")
}

/// One process per GPU (include/needle_hip.h, "multi-GPU").  What upstream does with rayon inside one process
/// (analyzer.rs:437-445 over videos, comparator.rs:549-564 over pairs) is spread over the ranks of a communicator
/// inside libneedle_capi.so: RCCL all-gathers on the library's own streams, no host round trips inside a job.
pub mod multi_gpu {
    use super::{check, ffi, ChannelMix, Comparator, Result, Sample, SampleFormat, SearchResult};
    use std::os::raw::c_int;
    use std::time::Duration;

    pub const COMM_ID_BYTES: usize = 128;

    /// Rank 0: the id every other rank needs (hand it over by file, socket, MPI ...).
    pub fn create_id() -> Result<[u8; COMM_ID_BYTES]> {
        let mut id = [0u8; COMM_ID_BYTES];
        unsafe { check(ffi::needle_hip_comm_create_id(id.as_mut_ptr()))? };
        Ok(id)
    }

    /// Collective over all ranks; binds `device` to this process first.
    pub fn init(id: &[u8; COMM_ID_BYTES], rank: usize, world_size: usize, device: usize) -> Result<()> {
        unsafe {
            check(ffi::needle_hip_set_device(device as c_int))?;
            check(ffi::needle_hip_comm_init(id.as_ptr(), rank as c_int, world_size as c_int))
        }
    }

    pub fn finalize() {
        unsafe { ffi::needle_hip_comm_finalize() }
    }

    /// The videos (or pairs) `rank` owns: `[first, first + count)`.
    pub fn shard(units: usize, world_size: usize, rank: usize) -> (usize, usize) {
        let (mut first, mut count) = (0usize, 0usize);
        unsafe { ffi::needle_hip_comm_shard(units, world_size as c_int, rank as c_int, &mut first, &mut count) };
        (first, count)
    }

    /// An analyze + search job over ALL videos of a library, this rank holding the PCM of its own block only.
    pub struct Library {
        raw: *mut ffi::NeedleHipLibrary,
        num_videos: usize,
        format: SampleFormat,
    }

    impl Library {
        pub fn new(num_videos: usize, opening_search_percentage: f32, hash_duration: Duration) -> Result<Self> {
            let mut raw = std::ptr::null_mut();
            unsafe {
                check(ffi::needle_hip_library_new(num_videos, opening_search_percentage, hash_duration.as_secs_f32(), &mut raw))?
            };
            Ok(Library { raw, num_videos, format: SampleFormat::S16 })
        }

        /// The sample rate of the PCM `load_pcm` and `rank_videos` will be given (2000..768000 Hz, default 11025): the
        /// windows are cut at that rate and resampled to 11025 Hz mono on the device on the way in
        /// (`needle_hip_library_set_sample_rate`).  Call before `load_pcm`.
        pub fn set_sample_rate(&mut self, sample_rate: u32) -> Result<&mut Self> {
            let rate = c_int::try_from(sample_rate).unwrap_or(c_int::MAX);
            unsafe { check(ffi::needle_hip_library_set_sample_rate(self.raw, rate))? };
            Ok(self)
        }

        /// A library of many shows: a label per video (only compared); only pairs inside a group are searched, and pair
        /// counts, pair ranges and `NeedleHipRun.problem` are grouped pair ids (`needle_hip_library_set_groups`).  Call
        /// before loading PCM; every rank passes the same labels.
        pub fn set_groups(&mut self, labels: &[u32]) -> Result<&mut Self> {
            unsafe { check(ffi::needle_hip_library_set_groups(self.raw, labels.as_ptr(), labels.len()))? };
            Ok(self)
        }

        /// The labels of a grouped library, one per video (an error on a plain one).
        pub fn groups(&self) -> Result<Vec<u32>> {
            let mut labels = vec![0u32; self.num_videos];
            unsafe { check(ffi::needle_hip_library_groups(self.raw, labels.as_mut_ptr(), labels.len()))? };
            Ok(labels)
        }

        /// The PCM loaded afterwards is folded to mono with `mix` on the way in (`needle_hip_library_set_channel_mix`;
        /// `None`: the plain average again).  Call before loading.
        pub fn set_channel_mix(&mut self, mix: Option<&ChannelMix>) -> Result<&mut Self> {
            let ptr = mix.map_or(std::ptr::null(), |m| m as *const ChannelMix);
            unsafe { check(ffi::needle_hip_library_set_channel_mix(self.raw, ptr))? };
            Ok(self)
        }

        /// The sample format of the PCM `load_pcm_format` will be given (`needle_hip_library_set_sample_format`; default
        /// s16, what `load_pcm` takes).  Call before loading.
        pub fn set_sample_format(&mut self, format: SampleFormat) -> Result<&mut Self> {
            unsafe { check(ffi::needle_hip_library_set_sample_format(self.raw, format as c_int))? };
            self.format = format;
            Ok(self)
        }

        /// A format per video and, optionally, a mix per video (`channels == 0`: the plain average) instead of the three
        /// setters above, which it excludes (`needle_hip_library_set_video_formats`).  Call before loading; `rank_videos`
        /// and `load_pcm_formats` then take `channels == 0`.
        pub fn set_video_formats(&mut self, formats: &[ffi::NeedleHipLaneFormat], mixes: Option<&[ffi::NeedleHipChannelMix]>) -> Result<&mut Self> {
            assert!(formats.len() == self.num_videos && mixes.map_or(true, |m| m.len() == self.num_videos));
            let mix_ptr = mixes.map_or(std::ptr::null(), |m| m.as_ptr());
            unsafe { check(ffi::needle_hip_library_set_video_formats(self.raw, formats.as_ptr(), mix_ptr))? };
            Ok(self)
        }

        /// The format of a video of a library that has formats (`needle_hip_library_video_format`).
        pub fn video_format(&self, video: usize) -> Result<ffi::NeedleHipLaneFormat> {
            let mut f = ffi::NeedleHipLaneFormat::default();
            unsafe { check(ffi::needle_hip_library_video_format(self.raw, video, &mut f))? };
            Ok(f)
        }

        /// `load_pcm` of a library with a format per video: `planes` is the concatenation of every video's planes as raw
        /// pointers (one for an interleaved video, `channels` for a planar one; all null for a video another rank owns)
        /// and `num_values[v]` counts video v's own values.
        ///
        /// # Safety
        /// Every non-null plane must hold the samples the video's format and `num_values` describe.
        pub unsafe fn load_pcm_formats(&mut self, planes: &[*const std::os::raw::c_void], num_values: &[usize], resident: bool) -> Result<()> {
            assert!(num_values.len() == self.num_videos);
            let mut expected = 0usize;
            for v in 0..self.num_videos {
                let f = self.video_format(v)?;
                expected += if f.format >= 5 { f.channels.max(1) as usize } else { 1 };
            }
            assert_eq!(planes.len(), expected, "one pointer per plane of every video");
            let ptrs = planes.as_ptr() as *const *const i16;
            if resident {
                check(ffi::needle_hip_library_set_pcm(self.raw, ptrs, num_values.as_ptr(), 0))
            } else {
                check(ffi::needle_hip_library_stream_pcm(self.raw, ptrs, num_values.as_ptr(), 0))
            }
        }

        /// The videos `[first, first + count)` whose PCM rank `rank` of `world_size` has to hold: the fingerprinting
        /// is cut by hashes (equal blocks of the arena), not by videos, so no rank idles; a pure function of the
        /// library's parameters and the stream lengths (`needle_hip_library_rank_videos`).
        pub fn rank_videos(&self, num_values: &[usize], channels: usize, world_size: usize, rank: usize) -> Result<(usize, usize)> {
            assert!(num_values.len() == self.num_videos);
            let (mut first, mut count) = (0usize, 0usize);
            unsafe {
                check(ffi::needle_hip_library_rank_videos(
                    self.raw,
                    num_values.as_ptr(),
                    channels as c_int,
                    world_size as c_int,
                    rank as c_int,
                    &mut first,
                    &mut count,
                ))?
            };
            Ok((first, count))
        }

        /// `pcm[v]` is `None` for the videos another rank owns; `num_values[v]` is known to every rank.
        /// `resident`: keep the PCM in HBM (repeatable analyze) instead of streaming it through.
        pub fn load_pcm(&mut self, pcm: &[Option<&[i16]>], num_values: &[usize], channels: usize, resident: bool) -> Result<()> {
            assert!(pcm.len() == self.num_videos && num_values.len() == self.num_videos);
            let ptrs: Vec<*const i16> = pcm.iter().map(|p| p.map_or(std::ptr::null(), |s| s.as_ptr())).collect();
            unsafe {
                if resident {
                    check(ffi::needle_hip_library_set_pcm(self.raw, ptrs.as_ptr(), num_values.as_ptr(), channels as c_int))
                } else {
                    check(ffi::needle_hip_library_stream_pcm(self.raw, ptrs.as_ptr(), num_values.as_ptr(), channels as c_int))
                }
            }
        }

        /// `load_pcm` in the format chosen with `set_sample_format` (it must be `T`'s interleaved or planar one): the samples
        /// are converted to s16 on the device on the way in.  Planar: `pcm` holds `channels` planes per video, one after
        /// the other, all `None` for a video another rank owns.
        pub fn load_pcm_format<T: Sample>(&mut self, pcm: &[Option<&[T]>], num_values: &[usize], channels: usize, resident: bool) -> Result<()> {
            let planar = self.format == T::PLANAR && self.format != T::INTERLEAVED;
            assert!(planar || self.format == T::INTERLEAVED, "set_sample_format first");
            let planes = if planar { channels.max(1) } else { 1 };
            assert!(pcm.len() == self.num_videos * planes && num_values.len() == self.num_videos);
            let ptrs: Vec<*const i16> = pcm.iter().map(|p| p.map_or(std::ptr::null(), |s| s.as_ptr() as *const i16)).collect();
            unsafe {
                if resident {
                    check(ffi::needle_hip_library_set_pcm(self.raw, ptrs.as_ptr(), num_values.as_ptr(), channels as c_int))
                } else {
                    check(ffi::needle_hip_library_stream_pcm(self.raw, ptrs.as_ptr(), num_values.as_ptr(), channels as c_int))
                }
            }
        }

        /// `Comparator::run_with_frame_hashes` across the communicator: the same `Vec<Option<SearchResult>>` on every rank.
        pub fn run<P: AsRef<std::path::Path>>(&mut self, comparator: &Comparator<P>) -> Result<Vec<Option<SearchResult>>> {
            let handle = comparator.handle()?;
            let mut results = vec![ffi::NeedleHipSearchResult::default(); self.num_videos];
            let status = unsafe {
                check(ffi::needle_hip_library_job_begin(self.raw, handle, 0)).and_then(|_| {
                    check(ffi::needle_hip_library_job_end(self.raw, handle, 0, results.as_mut_ptr(), std::ptr::null_mut()))
                })
            };
            unsafe { ffi::needle_audio_comparator_free(handle) };
            status?;
            let span = |a: u64, b: u64| (Duration::from_nanos(a), Duration::from_nanos(b));
            Ok(results
                .into_iter()
                .map(|r| {
                    r.has_result.then(|| SearchResult {
                        opening: r.has_opening.then(|| span(r.opening_start_ns, r.opening_end_ns)),
                        ending: r.has_ending.then(|| span(r.ending_start_ns, r.ending_end_ns)),
                    })
                })
                .collect())
        }
    }

    impl Library {
        /// The matched segments of every pair -- all ranks' shares -- that the last `run` worked from (a copy).
        pub fn last_runs(&self) -> Result<Vec<ffi::NeedleHipRun>> {
            let (mut ptr, mut n) = (std::ptr::null(), 0usize);
            unsafe { check(ffi::needle_hip_library_job_runs(self.raw, 0, &mut ptr, &mut n))? };
            Ok(if n == 0 { Vec::new() } else { unsafe { std::slice::from_raw_parts(ptr, n) }.to_vec() })
        }

        /// Both transforms (f32 first pass, f64 kernel) over this rank's resident PCM, every kept item compared on the
        /// device: `mismatches` and `accepted_mismatches` must be 0 (`needle_hip_library_audit`).
        pub fn audit(&mut self) -> Result<ffi::NeedleHipCertAudit> {
            let mut a = ffi::NeedleHipCertAudit::default();
            unsafe { check(ffi::needle_hip_library_audit(self.raw, &mut a))? };
            Ok(a)
        }
    }

    impl Drop for Library {
        fn drop(&mut self) {
            unsafe { ffi::needle_hip_library_free(self.raw) }
        }
    }
}
