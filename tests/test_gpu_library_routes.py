"""Every way PCM enters a resident library on the MI355X, one case per route of set_pcm / set_pcm_device: which landing
kernel a library's windows get (none, the down-mix, the conversion, the rematrix, the ingest) and what the resampler
reads behind it.  Two videos of about 20 s per route, built as tests/test_gpu_library_formats.py builds its season; the
windows' frame counts are neither multiples of 16 nor of a resampler tile and the device buffers lie one sample past a
16-byte boundary -- the smallest shapes at which a wrong piece boundary, a wrong channel count at the resampler or a
wrong staging offset shows.  Each route runs whole and with a staging limit of 3001 and of 1000 values (one tile per
piece; the 11025 Hz windows in 16-frame groups by the hundred).  The hashes are the oracle's, bit-exact, for every video
and both regions; whole runs also pin the launches of every landing kernel and of the resampler."""
import pytest

from needle_amd import capi
from oracle import oracle as O
from tests.test_gpu_library_formats import MASK_51, Season, launches_of
from tests.test_gpu_library_rates import ENDING, hashes_of, job, oracle_hashes, windows

pytestmark = pytest.mark.gpu
SECONDS = (20.37, 19.61)

# route -> (channels, rate, format, mask of the library-wide mix, a format per video?, launches of one whole load)
ROUTES = {
    "direct": (2, 11025, capi.SAMPLE_S16, None, False, {}),                          # one upload, or device-to-device copies
    "downmix": (6, 11025, capi.SAMPLE_S16, None, False, {"downmix": 1}),
    "raw-resampled": (2, 48000, capi.SAMPLE_S16, None, False, {"resample": 1}),       # the resampler reads the raw stereo
    "convert-stereo": (2, 11025, capi.SAMPLE_S32, None, False, {"convert": 1}),       # stereo stays resident
    "convert-surround": (6, 48000, capi.SAMPLE_F32P, None, False, {"convert": 1, "resample": 1}),
    "mix": (6, 11025, capi.SAMPLE_S16, MASK_51, False, {"rematrix": 1}),
    "formats": (None, None, None, None, True, {"ingest": 1, "resample": 2}),
}
VIDEO_FORMATS = [(2, 44100, capi.SAMPLE_S16), (6, 48000, capi.SAMPLE_F32P)]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert capi.device_count() > 0, "GPU tests need a HIP device (the product has no CPU fallback)"


@pytest.fixture(scope="module")
def seasons():
    """route -> its two videos with the oracle's frame hashes, computed once."""
    out = {}
    for k, (route, (ch, rate, fmt, mask, per_video, _)) in enumerate(ROUTES.items()):
        formats = VIDEO_FORMATS if per_video else [(ch, rate, fmt)] * 2
        season = Season([f + (None if per_video else mask, s) for f, s in zip(formats, SECONDS)], seed=10 * k)
        for n_values, (c, r, _) in zip(season.lens, season.formats):
            tile = capi.resample_plan(r)["tile_outputs"] if r != 11025 else 1
            for _, frames, *_ in windows(n_values, c, r):
                assert frames % 16 and (tile == 1 or O.lib().ora_resample_out_len(frames, r) % tile), (route, frames)
        out[route] = season
    return out


def new_library(route):
    ch, rate, fmt, mask, per_video, _ = ROUTES[route]
    lib = capi.Library(2).include_endings(ENDING)
    if per_video:
        return lib.set_video_formats(VIDEO_FORMATS), 0
    if rate != 11025:
        lib.set_sample_rate(rate)
    if fmt != capi.SAMPLE_S16:
        lib.set_sample_format(fmt)
    if mask is not None:
        lib.set_channel_mix(capi.channel_mix_default(mask))
    return lib, ch


def load(season, lib, door, channels):
    if door == "set_pcm":
        lib.set_pcm(season.streams, season.lens, channels=channels)
    else:
        bufs, ptrs = season.device_copies()
        lib.set_pcm_device(ptrs, season.lens, channels=channels)
        del bufs                                                                   # the caller's buffers are free on return


@pytest.mark.parametrize("limit", [None, 3001, 1000], ids=["whole", "3001", "1000"])
@pytest.mark.parametrize("door", ["set_pcm", "set_pcm_device"])
@pytest.mark.parametrize("route", list(ROUTES))
def test_route(seasons, monkeypatch, route, door, limit):
    season = seasons[route]
    lib, channels = new_library(route)
    if limit is None:
        got = launches_of(lambda: load(season, lib, door, channels))
        want = dict.fromkeys(("ingest", "rematrix", "resample", "convert", "downmix"), 0)
        want.update(ROUTES[route][5])
        assert got == want, got
    else:                               # the number of batches is the plan's own: only what lands is pinned
        monkeypatch.setenv("NEEDLE_HIP_MAX_BATCH_VALUES", str(limit))
        load(season, lib, door, channels)
    job(lib, capi.Comparator(season.names, include_endings=True, min_opening_duration=5, min_ending_duration=3))
    for v in range(season.n):
        assert hashes_of(lib.frame_hashes(v)) == oracle_hashes(season.ref[v]), v
        assert len(season.ref[v].opening) > 20 and len(season.ref[v].ending) > 5
    audit = lib.audit()
    assert audit["mismatches"] == 0 and audit["accepted_mismatches"] == 0
    assert audit["items"] == sum(len(f.opening) + len(f.ending) for f in season.ref)
