"""The weights file (host/weights.h) through the host-only entry points gcnhost_weights_write / gcnhost_weights_read and
model.read_weights / write_weights: no GPU needed."""
import ctypes as C
import struct
import zlib

import numpy as np
import pytest

from cuda_gcn_amd import _lib, model


def _weights(F=13, h=5, c=3, seed=0):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((F, h)).astype(np.float32), rng.standard_normal((h, c)).astype(np.float32)


def _write(path, w1, w2):
    lib = _lib.gcnhost()
    F, h = w1.shape
    c = w2.shape[1]
    return lib.gcnhost_weights_write(str(path).encode(), F, h, c, np.ascontiguousarray(w1).ctypes.data, np.ascontiguousarray(w2).ctypes.data)


def _read(path, F, h, c, shape_only=False):
    lib = _lib.gcnhost()
    a, b, d = C.c_int(F), C.c_int(h), C.c_int(c)
    w1 = np.zeros((max(F, 1), max(h, 1)), np.float32)
    w2 = np.zeros((max(h, 1), max(c, 1)), np.float32)
    rc = lib.gcnhost_weights_read(str(path).encode(), C.byref(a), C.byref(b), C.byref(d),
                                  None if shape_only else w1.ctypes.data, None if shape_only else w2.ctypes.data)
    return rc, (a.value, b.value, d.value), w1, w2, lib.gcnhost_last_error().decode()


def test_round_trip_is_bit_exact(tmp_path):
    w1, w2 = _weights()
    w1[0, 0], w1[1, 1], w2[0, 0] = -0.0, np.float32(1e-45), np.float32(3.4e38)     # signed zero, a subnormal, a large value
    p = tmp_path / "w.gcnw"
    assert _write(p, w1, w2) == 0
    rc, dims, r1, r2, _ = _read(p, 13, 5, 3)
    assert rc == 0 and dims == (13, 5, 3)
    assert r1.tobytes() == w1.tobytes() and r2.tobytes() == w2.tobytes()


def test_header_holds_the_widths_little_endian(tmp_path):
    w1, w2 = _weights(7, 4, 2)
    p = tmp_path / "w.gcnw"
    assert _write(p, w1, w2) == 0
    raw = p.read_bytes()
    assert raw[:4] == b"GCNW"
    version, F, h, c = struct.unpack("<Iiii", raw[4:20])
    assert version == 1 and (F, h, c) == (7, 4, 2)
    assert len(raw) == 20 + 4 * (7 * 4 + 4 * 2) + 4
    assert raw[20:20 + 4 * 28] == w1.astype("<f4").tobytes()
    assert struct.unpack("<I", raw[-4:])[0] == zlib.crc32(raw[:-4])           # IEEE CRC-32 of everything before it
    rc, dims, *_ = _read(p, 0, 0, 0, shape_only=True)
    assert rc == 0 and dims == (7, 4, 2)


def _corrupt(p, fn):
    raw = bytearray(p.read_bytes())
    p.write_bytes(bytes(fn(raw)))


@pytest.mark.parametrize("damage,needle", [
    (lambda r: r[:-1], "truncated"),
    (lambda r: r[:30], "truncated"),
    (lambda r: r[:10], "GCNW"),
    (lambda r: b"", "GCNW"),
    (lambda r: r + b"\0", "truncated"),
    (lambda r: b"XCNW" + r[4:], "GCNW"),
    (lambda r: r[:4] + struct.pack("<I", 2) + r[8:], "version 2"),
    (lambda r: r[:40] + bytes([r[40] ^ 1]) + r[41:], "CRC"),
    (lambda r: r[:8] + struct.pack("<i", -3) + r[12:], "not positive"),
    (lambda r: r[:8] + struct.pack("<iii", 1 << 30, 1 << 30, 1 << 30) + r[20:], "truncated"),
])
def test_bad_files_are_refused(tmp_path, damage, needle):
    w1, w2 = _weights()
    p = tmp_path / "w.gcnw"
    assert _write(p, w1, w2) == 0
    _corrupt(p, damage)
    for shape_only in (True, False):
        rc, _, r1, r2, err = _read(p, 13, 5, 3, shape_only)
        assert rc != 0 and needle in err, err
        assert not r1.any() and not r2.any()                                   # nothing copied out
    with pytest.raises(model.GcnHostError):
        model.read_weights(str(p))


@pytest.mark.parametrize("dims", [(12, 5, 3), (13, 6, 3), (13, 5, 4)])
def test_widths_that_do_not_match_the_buffers_are_refused(tmp_path, dims):
    w1, w2 = _weights()
    p = tmp_path / "w.gcnw"
    assert _write(p, w1, w2) == 0
    rc, _, r1, r2, err = _read(p, *dims)
    assert rc != 0 and "input_dim=13 hidden_dim=5 output_dim=3" in err, err
    assert not r1.any() and not r2.any()


def test_missing_file_and_bad_arguments(tmp_path):
    rc, _, _, _, err = _read(tmp_path / "nothing.gcnw", 1, 1, 1)
    assert rc != 0 and "cannot open" in err
    w1, w2 = _weights()
    lib = _lib.gcnhost()
    assert lib.gcnhost_weights_write(str(tmp_path / "x").encode(), 0, 5, 3, w1.ctypes.data, w2.ctypes.data) != 0
    assert lib.gcnhost_weights_write(str(tmp_path / "no_dir" / "x").encode(), 13, 5, 3, w1.ctypes.data, w2.ctypes.data) != 0


def test_model_read_weights_returns_the_same_arrays(tmp_path):
    w1, w2 = _weights(602, 128, 41, seed=3)
    p = tmp_path / "w.gcnw"
    model.write_weights(str(p), w1, w2)
    r1, r2 = model.read_weights(str(p))
    assert r1.dtype == np.float32 and r1.shape == (602, 128) and r2.shape == (128, 41)
    assert np.array_equal(r1, w1) and np.array_equal(r2, w2)
    with pytest.raises(ValueError):
        model.write_weights(str(p), w1, w2.T)
