"""CPU-only checks of the drop-in boundary: the C-ABI library loads and exports
every symbol include/gcnhip.h declares (no compute calls: there is no GPU here)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_functions(path):
    txt = open(path).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(gcn(?:hip|host)_\w+)\s*\(", txt)))


def test_gcnhip_exports_the_symbols_of_both_headers():
    """gcnhip.h = the 1:1 surface a binding into the reference calls; gcnhip_driver.h = the protocol of this
    repository's host driver.  The library exports both sets and the python binding table covers them exactly."""
    from cuda_gcn_amd import _lib
    lib = _lib.gcnhip()
    names = header_functions(os.path.join(ROOT, "include", "gcnhip.h"))
    assert 40 <= len(names) <= 60, len(names)                       # the reference's wrappers 1:1, not the driver's variants
    for n in names:
        assert hasattr(lib, n), f"{n} declared in gcnhip.h but not exported"
    drv = [n for n in header_functions(os.path.join(ROOT, "include", "gcnhip_driver.h")) if n not in names]
    assert len(drv) >= 30
    for n in drv:
        assert hasattr(lib, n), f"{n} declared in gcnhip_driver.h but not exported"
    assert sorted(_lib.GCNHIP_SYMBOLS) == sorted(names + drv)


def test_integration_binding_needs_only_the_stable_header():
    """every gcnhip_* call INTEGRATION.md's section B shows in the reference-side binding is declared in gcnhip.h itself"""
    txt = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    a = txt.index("## B")
    nxt = txt.find("\n## ", a + 5)
    sect = txt[a:nxt if nxt > 0 else len(txt)]
    code = "\n".join(re.findall(r"```(?:cpp|c\+\+|c)?\n(.*?)```", sect, flags=re.S))
    used = set(re.findall(r"\b(gcnhip_\w+)\s*\(", code))
    stable = set(header_functions(os.path.join(ROOT, "include", "gcnhip.h")))
    assert used and used <= stable, sorted(used - stable)


def test_error_strings_without_gpu():
    from cuda_gcn_amd import _lib
    lib = _lib.gcnhip()
    assert b"invalid argument" in lib.gcnhip_error_string(-1)
    assert lib.gcnhip_version().startswith(b"gcnhip")


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    from cuda_gcn_amd import _lib
    monkeypatch.setattr(_lib, "LIBDIR", str(tmp_path))
    monkeypatch.setattr(_lib, "_cache", {})
    with pytest.raises(_lib.NativeLibraryMissing):
        _lib._load("libgcnhip.so")


def test_no_gpu_means_error_not_fallback():
    """on a box without a GPU the product path must raise, never compute on the CPU"""
    from cuda_gcn_amd import _lib
    lib = _lib.gcnhip()
    n = ctypes.c_int(-1)
    rc = lib.gcnhip_device_count(ctypes.byref(n))
    if rc == 0 and n.value > 0:
        pytest.skip("a GPU is present")
    from cuda_gcn_amd.ops import Device, GcnHipError
    with pytest.raises(GcnHipError):
        Device(0)
