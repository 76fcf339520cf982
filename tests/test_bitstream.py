"""CPU: the container of one compressed image (icm_amd/bitstream.py).  pack / unpack round trips at the edges of every
field, and unpack refuses -- with ValueError and nothing else -- every truncation, every single-byte change, appended
bytes and unknown version / architecture ids."""
import struct
import subprocess
import sys
import zlib

import pytest

from icm_amd import bitstream as B

HDR = {"arch": "cnn", "height": 175, "width": 201, "pads": (27, 28, 8, 9), "shape": (3, 4), "fingerprint": 0xDEADBEEF}


def _recrc(body: bytes) -> bytes:
    return body + struct.pack("<I", zlib.crc32(body) & 0xFFFFFFFF)


@pytest.mark.parametrize("header,strings", [
    (HDR, [b"\x01\x02\x03\x04\x05", b"\xff\x00"]),
    (HDR, [b"", b""]),
    (HDR, [b"", b"x"]),
    (HDR, [b"y", b"z"]),
    (HDR, [bytes(range(256)) * 4096, b"tail"]),                      # a 1 MB string
    ({**HDR, "height": 1, "width": 1, "pads": (31, 32, 31, 32), "shape": (1, 1)}, [b"a", b"b"]),
    ({"arch": "stf", "height": 2 ** 32 - 1, "width": 2 ** 32 - 1, "pads": (65535,) * 4, "shape": (65535, 65535),
      "fingerprint": 2 ** 32 - 1}, [b"q" * 7, b""]),                 # the largest values the fields hold
    ({**HDR, "fingerprint": 0, "pads": (0, 0, 0, 0)}, []),
    (HDR, [b"a", b"bb", b"ccc"]),
])
def test_pack_unpack_round_trip(header, strings):
    data = B.pack(header, strings)
    assert isinstance(data, bytes)
    assert len(data) == B.FIXED_BYTES + 4 * len(strings) + sum(map(len, strings)) + B.CRC_BYTES
    h, s = B.unpack(data)
    assert h == header and s == list(strings)
    assert B.unpack(bytearray(data)) == (h, s)


def test_header_size_constant():
    assert B.HEADER_BYTES_2 == len(B.pack(HDR, [b"", b""])) == 46
    assert len(B.pack(HDR, [b"abc", b"de"])) == B.HEADER_BYTES_2 + 5


def test_layout_is_the_documented_one():
    data = B.pack(HDR, [b"abc", b"de"])
    assert data[:4] == b"ICMB"
    assert struct.unpack_from("<HHII4H2HIH", data, 4) == (1, 0, 175, 201, 27, 28, 8, 9, 3, 4, 0xDEADBEEF, 2)
    assert struct.unpack_from("<II", data, 34) == (3, 2) and data[42:47] == b"abcde"
    assert struct.unpack_from("<I", data, 47)[0] == zlib.crc32(data[:47])


def test_every_proper_prefix_is_refused():
    data = B.pack(HDR, [b"\x01\x02\x03\x04\x05" * 6, b"\xff\x00" * 10])
    for n in range(len(data)):
        with pytest.raises(ValueError):
            B.unpack(data[:n])


def test_every_single_byte_change_is_refused():
    data = B.pack(HDR, [b"\x01\x02\x03\x04\x05" * 6, b"\xff\x00" * 10])
    assert 90 <= len(data) <= 110
    for i in range(len(data)):
        for delta in (1, 0x80, 0xFF):
            bad = bytearray(data)
            bad[i] = (bad[i] + delta) & 0xFF
            with pytest.raises(ValueError):
                B.unpack(bytes(bad))


def test_appended_bytes_are_refused():
    data = B.pack(HDR, [b"abc", b"de"])
    for extra in (b"\x00", b"ICMB", data):
        with pytest.raises(ValueError, match="trailing"):
            B.unpack(data + extra)


def test_unknown_version_and_architecture_are_named():
    body = bytearray(B.pack(HDR, [b"abc", b"de"])[:-4])
    v2 = bytearray(body)
    struct.pack_into("<H", v2, 4, 2)
    with pytest.raises(ValueError, match="version"):
        B.unpack(_recrc(bytes(v2)))
    a9 = bytearray(body)
    struct.pack_into("<H", a9, 6, len(B.ARCHS))
    with pytest.raises(ValueError, match="architecture"):
        B.unpack(_recrc(bytes(a9)))
    assert B.unpack(_recrc(bytes(body)))[1] == [b"abc", b"de"]       # the helper itself writes a valid CRC
    with pytest.raises(ValueError, match="magic"):
        B.unpack(_recrc(b"ICMX" + bytes(body[4:])))
    with pytest.raises(ValueError, match="CRC"):
        B.unpack(bytes(body) + b"\x00\x00\x00\x00")
    lie = bytearray(body)
    struct.pack_into("<I", lie, 34, 2 ** 32 - 1)                      # a length far past the data, CRC made to fit
    with pytest.raises(ValueError, match="past the data"):
        B.unpack(_recrc(bytes(lie)))
    many = bytearray(body)
    struct.pack_into("<H", many, 32, 65535)                           # a string count far past the data
    with pytest.raises(ValueError, match="past the data"):
        B.unpack(_recrc(bytes(many)))


def test_unpack_refuses_other_types_and_pack_refuses_bad_headers():
    for bad in (None, "ICMB", 7, [1, 2]):
        with pytest.raises(ValueError):
            B.unpack(bad)
    for patch in ({"arch": "stf6"}, {"height": 0}, {"width": 2 ** 32}, {"pads": (0, 0, 70000, 0)}, {"pads": (1, 2, 3)},
                  {"shape": (1, -1)}, {"fingerprint": -1}, {"height": 1.5}):
        with pytest.raises(ValueError):
            B.pack({**HDR, **patch}, [b"", b""])
    with pytest.raises(ValueError, match="lacks"):
        B.pack({k: v for k, v in HDR.items() if k != "shape"}, [])


def test_module_imports_without_the_shared_library(tmp_path):
    """a fresh interpreter with ICM_LIB pointing nowhere: the container needs neither the library nor torch"""
    import os
    pkg = os.path.dirname(os.path.dirname(os.path.abspath(B.__file__)))
    code = ("import sys; from icm_amd import bitstream as B; "
            "d = B.pack({'arch': 'cnn', 'height': 2, 'width': 3, 'pads': (30, 31, 31, 31), 'shape': (1, 1), "
            "'fingerprint': 5}, [b'ab', b'c']); assert B.unpack(d)[1] == [b'ab', b'c']; "
            "assert 'icm_amd._lib' not in sys.modules and 'torch' not in sys.modules; print('ok')")
    env = {**os.environ, "ICM_LIB": str(tmp_path / "missing.so"), "PYTHONPATH": pkg}
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr
