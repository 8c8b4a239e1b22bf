"""The feeder's audit at the boundary, without a GPU: needle_hip_feeder_set_audit / needle_hip_feeder_audit through every
layer (header, library, capi.py, ffi.rs, lib.rs), their NULL arguments, and the refusals that are decided on the host
before any device work: `audit` while the audit is off, a lane out of range, and NEEDLE_HIP_STFT=f64."""
import ctypes as C
import inspect
import os
import re

from needle_amd import capi
from tests import rust_ffi_check as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["needle_hip_feeder_set_audit", "needle_hip_feeder_audit"]
INVALID, NULL = capi.ERROR_NAMES.index("InvalidArgument"), capi.ERROR_NAMES.index("NullArgument")


def test_both_symbols_in_every_layer():
    header = R.strip_comments(open(os.path.join(ROOT, "include", "needle_hip.h")).read())
    lib_rs = open(os.path.join(ROOT, "rust", "needle-hip", "src", "lib.rs")).read()
    protos = R.c_prototypes()
    fns, _, _ = R.rust_declarations()
    L = capi.lib()
    for sym in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % sym, header), sym
        assert hasattr(L, sym), sym
        assert sym in capi.NEEDLE_HIP_H_SYMBOLS, sym
        assert sym in fns, f"{sym} is not declared in ffi.rs"
        assert fns[sym] == protos[sym], (sym, fns[sym], protos[sym])
        assert "ffi::%s(" % sym in lib_rs, f"{sym} is not used by lib.rs"
    assert protos["needle_hip_feeder_set_audit"] == (["*mut NeedleHipFeeder", "bool"], "NeedleError")
    assert protos["needle_hip_feeder_audit"] == (["*mut NeedleHipFeeder", "usize", "*mut NeedleHipCertAudit"], "NeedleError")
    assert "pub fn set_audit(&mut self, on: bool) -> Result<()>" in lib_rs
    assert "pub fn audit(&mut self, lane: Option<usize>) -> Result<ffi::NeedleHipCertAudit>" in lib_rs


def test_python_wrappers_have_the_stated_signatures():
    s = inspect.signature(capi.Feeder.set_audit)
    assert list(s.parameters) == ["self", "on"]
    a = inspect.signature(capi.Feeder.audit)
    assert list(a.parameters) == ["self", "lane"] and a.parameters["lane"].default is None
    assert [k for k, _ in capi.CCertAudit._fields_] == ["items", "accepted", "accepted_mismatches", "mismatches",
                                                        "max_error_over_s", "max_s"]


def test_null_arguments_and_host_side_refusals(monkeypatch):
    L = capi.lib()
    monkeypatch.delenv("NEEDLE_HIP_STFT", raising=False)
    a = capi.CCertAudit()
    assert L.needle_hip_feeder_set_audit(None, True) == NULL and L.needle_hip_feeder_set_audit(None, False) == NULL
    assert L.needle_hip_feeder_audit(None, 0, C.byref(a)) == NULL
    f = capi.Feeder(3, 1, 11025, capi.SAMPLE_S16, 2)
    assert L.needle_hip_feeder_audit(f._h, 0, None) == NULL
    # the audit is off: InvalidArgument, for a lane, for all lanes and for a lane out of range alike; the struct untouched
    a.items = 7
    for lane in (0, 2, 3, capi.Feeder.NO_LANE):
        assert L.needle_hip_feeder_audit(f._h, lane, C.byref(a)) == INVALID
    assert a.items == 7
    f.set_audit(False)                                            # off -> off on a new feeder: nothing to do, no device
    # NEEDLE_HIP_STFT=f64 has no first pass to audit: refused before any device work
    monkeypatch.setenv("NEEDLE_HIP_STFT", "f64")
    assert L.needle_hip_feeder_set_audit(f._h, True) == INVALID
    assert b"f64" in (L.needle_hip_last_error_message() or b"")
    assert L.needle_hip_feeder_audit(f._h, 0, C.byref(a)) == INVALID   # ... and it stayed off
    monkeypatch.delenv("NEEDLE_HIP_STFT")
    kept, fed, fin = f.ready(1)
    assert (kept, fed, fin) == (0, 0, False)
