"""The host half of the JPEG route, without a GPU.

tests/jpeg_host_main.cpp - a stand-alone program around csrc/jpeg_host.h and csrc/jpeg_math.h - is built here with g++ under
AddressSanitizer and UBSan (a plain build only when the sanitizer link itself fails; the program prints which build ran) and
decodes whole files on the host by looping the functions the device kernels are made of.  Expected pixels: g19_jpeg.npz
(tests/golden/make_golden_jpeg.py), i.e. PIL's decode, which is libjpeg's - every byte must be equal.  The same program decodes
every truncation and 2000 seeded one-byte mutations of two fixtures: each decode must end in a status and the sanitizers stay
silent.  The header parse, the colour-space rule of the markers and image_size are checked through the ctypes binding, which
needs no GPU for these calls."""
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CSRC = os.path.join(ROOT, "sw-nerf_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "g19_jpeg.npz")
CAMERA_DIR = "/root/reference/2d_pos_encoding/src"
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


@pytest.fixture(scope="module")
def g19():
    return dict(np.load(GOLDEN, allow_pickle=False))


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("jpeg_host") / "jpeg_host_main")
    base = ["g++", "-O1", "-g", "-std=c++17", "-I", CSRC, os.path.join(ROOT, "tests", "jpeg_host_main.cpp"), "-o", exe]
    r = subprocess.run(base + SAN, capture_output=True, text=True)
    if r.returncode != 0:
        assert "sanitize" in r.stderr or "asan" in r.stderr or "ubsan" in r.stderr, r.stderr      # only a failed sanitizer link falls back
        subprocess.run(base, check=True)
    return exe


def _run(program, *args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([program, *args], capture_output=True, text=True, timeout=300, env=env)
    print(r.stdout[-6000:], r.stderr[-3000:])
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    return r


def _names(g19):
    return [str(n) for n in g19["names"]]


def _write_fixtures(g19, d):
    lines = []
    for n in _names(g19):
        jpg = os.path.join(d, n + ".jpg")
        with open(jpg, "wb") as f:
            f.write(g19[n + "_jpg"].tobytes())
        if n.endswith("_prog"):
            lines.append(f"{jpg} -")
        else:
            with open(os.path.join(d, n + ".rgb"), "wb") as f:
                f.write(np.ascontiguousarray(g19[n + "_rgb"]).tobytes())
            lines.append(f"{jpg} {os.path.join(d, n + '.rgb')}")
    return lines


def test_fixture_set_is_the_one_the_cases_need(g19):
    names = _names(g19)
    assert len(names) == 21 and sum(n.endswith("_prog") for n in names) == 1
    for want in ("1x1_420", "2x3_422", "2x3_420", "5x4_422", "5x4_420", "6x5_420", "9x35_gray", "40x56_420_rst2", "17x23_420_prog"):
        assert want in names
    for hw in ("17x23", "16x16", "33x9"):
        for s in ("444", "422", "420"):
            assert f"{hw}_{s}" in names
    assert b"\xff\xdd" in g19["40x56_420_rst2_jpg"].tobytes() and b"\xff\xd0" in g19["40x56_420_rst2_jpg"].tobytes()
    assert b"\xff\xc2" in g19["17x23_420_prog_jpg"].tobytes()
    assert os.path.getsize(GOLDEN) < 200 * 1024
    assert str(g19["pil_version"]) and "jpeg" in str(g19["libjpeg_version"])


def test_host_decode_of_every_fixture_equals_libjpeg(program, g19, tmp_path):
    lines = _write_fixtures(g19, str(tmp_path))
    with open(tmp_path / "list.txt", "w") as f:
        f.write("\n".join(lines) + "\n")
    r = _run(program, "check", str(tmp_path / "list.txt"))
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert r.stdout.count("0 of ") == len(lines) - 1 and "MISMATCH" not in r.stdout and "EXPECTED" not in r.stdout
    assert "17x23_420_prog.jpg: status 1" in r.stdout


def test_truncations_and_mutations_end_in_a_status(program, g19, tmp_path):
    _write_fixtures(g19, str(tmp_path))
    files = [str(tmp_path / "17x23_420.jpg"), str(tmp_path / "40x56_420_rst2.jpg")]
    r = _run(program, "fuzz", "20261019", "2000", *files)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert r.stdout.count(" 2000 mutations: ") == 2 and r.stdout.count(" truncations: ") == 2
    for line in r.stdout.splitlines():
        if " truncations: " in line:                                                               # only a few of the longest cuts still decode
            assert int(line.split("truncations: ")[1].split(" decoded")[0]) <= 4, line
            assert int(line.split("here, ")[1].split(" corrupt")[0]) > 100, line


def test_camera_files_equal_pil(program, tmp_path):
    """files from a camera pipeline: Huffman tables other than PIL's, APPn segments"""
    paths = [os.path.join(CAMERA_DIR, f"{k}.jpg") for k in (1, 3, 4)]
    if not all(os.path.exists(p) for p in paths):
        pytest.skip("the camera pictures are not on this machine")
    Image = pytest.importorskip("PIL.Image")
    lines = []
    for k, p in enumerate(paths):
        with open(tmp_path / f"{k}.rgb", "wb") as f:
            f.write(np.ascontiguousarray(np.asarray(Image.open(p).convert("RGB"))).tobytes())
        lines.append(f"{p} {tmp_path / f'{k}.rgb'}")
    with open(tmp_path / "list.txt", "w") as f:
        f.write("\n".join(lines) + "\n")
    r = _run(program, "check", str(tmp_path / "list.txt"))
    assert r.returncode == 0 and r.stdout.count(" 0 of ") == 3, r.stdout[-2000:]


# ---- the ctypes binding: header parse, colour-space rule, image_size ------------------------------------------------------
def _segments(data):
    """[(marker, start, end)] of the segments between SOI and the entropy-coded data (end: one past the payload)"""
    out, p = [], 2
    while True:
        assert data[p] == 0xFF
        m, n = data[p + 1], (data[p + 2] << 8) | data[p + 3]
        out.append((m, p, p + 2 + n))
        p += 2 + n
        if m == 0xDA:
            return out


def _without(data, marker):
    for m, a, b in _segments(data):
        if m == marker:
            return data[:a] + data[b:]
    raise AssertionError(marker)


def _with_ids(data, ids):
    d = bytearray(data)
    for m, a, b in _segments(data):
        if m == 0xC0:
            for c in range(3):
                d[a + 10 + 3 * c] = ids[c]
        if m == 0xDA:
            for c in range(3):
                d[a + 5 + 2 * c] = ids[c]
    return bytes(d)


def _adobe(transform):
    return b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00" + bytes([transform])


def _header(data):
    from swnerf import images
    return images._jpeg_header(data, "test")


def test_header_reports_geometry_tables_and_restart_interval(g19):
    import ctypes
    from swnerf import _lib
    sampling = {"444": _lib.JPEG_444, "422": _lib.JPEG_422, "420": _lib.JPEG_420, "gray": _lib.JPEG_444}
    for n in _names(g19):
        data = g19[n + "_jpg"].tobytes()
        j = _header(data)
        if n.endswith("_prog"):
            assert j is None and b"not decodable here" in _lib.lib().swnerf_last_error()
            continue
        H, W = (int(v) for v in n.split("_")[0].split("x"))
        s = n.split("_")[1]
        assert (j.H, j.W, j.ncomp, j.sampling) == (H, W, 1 if s == "gray" else 3, sampling[s]), n
        hs, vs = {"444": (1, 1), "422": (2, 1), "420": (2, 2), "gray": (1, 1)}[s]
        mx, my = -(-W // (8 * hs)), -(-H // (8 * vs))
        assert j.ncoef == 64 * mx * my * (hs * vs + (0 if s == "gray" else 2)), n
        assert j.qt.shape == (64 * j.ncomp,) and j.qt.dtype == np.uint16
        coef = j.coefficients()
        assert coef.shape == (j.ncoef,) and coef.dtype == np.int16
    info = (ctypes.c_int32 * _lib.JPEG_INFO_LEN)()
    qt = np.zeros((_lib.JPEG_QT_LEN,), np.uint16)
    data = g19["40x56_420_rst2_jpg"].tobytes()
    assert _lib.lib().swnerf_jpeg_header(data, len(data), info, qt.ctypes.data) == 0
    assert list(info)[:5] == [40, 56, 3, _lib.JPEG_420, 2] and data[info[5] - 14:info[5] - 12] == b"\xff\xda"
    # quality 100: every divisor is 1.  Quality 30 scales Annex K's luminance table (16 11 10 ... / 12 12 14 ...) by 5000 / 30 = 166
    # per cent: (16 * 166 + 50) / 100 = 27, 18, 17 in the first row and (12 * 166 + 50) / 100 = 20 under the 27 - in ZIGZAG order
    # the 20 would be the third entry
    assert (_header(g19["24x16_420_q100_jpg"].tobytes()).qt == 1).all()
    q30 = _header(g19["24x16_420_q30_jpg"].tobytes()).qt
    assert q30[:3].tolist() == [27, 18, 17] and q30[8] == 20 and q30[64:67].tolist() == [(17 * 166 + 50) // 100, (18 * 166 + 50) // 100, (24 * 166 + 50) // 100]


def test_colour_space_rule_and_refusals(g19):
    from swnerf import _lib
    data = g19["17x23_444_jpg"].tobytes()
    assert [m for m, _, _ in _segments(data)][0] == 0xE0 and _header(data) is not None           # PIL writes JFIF
    bare = _without(data, 0xE0)
    assert _header(bare) is not None                                                              # ids 1, 2, 3: YCbCr
    rgb_ids = _with_ids(bare, b"RGB")
    assert _header(rgb_ids) is None and b"RGB" in _lib.lib().swnerf_last_error()
    assert _header(_with_ids(data, b"RGB")) is not None                                           # a JFIF marker decides first
    assert _header(data[:2] + _adobe(0) + bare[2:]) is None                                       # Adobe, transform 0: RGB
    assert _header(data[:2] + _adobe(1) + bare[2:]) is not None
    assert _header(data[:2] + _adobe(1) + rgb_ids[2:]) is not None                                # Adobe decides before the ids
    assert _header(data[:2] + b"\xff\xff\xff" + data[2:]) is not None                             # fill bytes before a marker
    sof = [a for m, a, _ in _segments(data) if m == 0xC0][0]
    for off, val in ((4, 12), (9, 4), (9, 2), (11, 0x41), (11, 0x12), (14, 0x21)):                # precision, components, samplings
        d = bytearray(data)
        d[sof + off] = val
        assert _header(bytes(d)) is None, (off, val)
    for cut in (0, 1, 2, 3, 20, sof + 6, [a for m, a, _ in _segments(data) if m == 0xDA][0] + 5):
        assert _header(data[:cut]) is None, cut
    assert _header(b"\xff\xd8\xff\xe0 no picture") is None
    # a cut inside the entropy-coded segment of an accepted file is an error that names the file
    j = _header(data[:len(data) - 200])
    with pytest.raises(ValueError, match="test.*truncated"):
        j.coefficients()
    # the same pixels whichever marker announced YCbCr
    a, b = _header(data).coefficients(), _header(bare).coefficients()
    assert np.array_equal(a, b)


def test_entropy_decode_from_several_threads(g19):
    data = g19["40x56_420_rst2_jpg"].tobytes()
    want = _header(data).coefficients()
    got = [None] * 6

    def work(k):
        got[k] = [_header(data).coefficients() for _ in range(20)]
    threads = [threading.Thread(target=work, args=(k,)) for k in range(6)]
    [t.start() for t in threads]
    [t.join() for t in threads]
    assert all(np.array_equal(c, want) for cs in got for c in cs)


def test_restart_markers_are_checked(g19):
    data = bytearray(g19["40x56_420_rst2_jpg"].tobytes())
    scan = [b for m, _, b in _segments(bytes(data)) if m == 0xDA][0]
    first = bytes(data).index(b"\xff\xd0", scan)
    data[first + 1] = 0xD3                                                                        # RST3 where RST0 belongs
    with pytest.raises(ValueError, match="RST0"):
        _header(bytes(data)).coefficients()


def test_image_size_and_pil_fallback(g19, tmp_path, monkeypatch):
    from swnerf import images
    for k in ("PIL", "PIL.Image"):
        monkeypatch.setitem(sys.modules, k, None)                                                 # `from PIL import Image` now raises ImportError
    for n in ("17x23_422", "9x35_gray"):
        p = str(tmp_path / (n + ".JPG"))
        with open(p, "wb") as f:
            f.write(g19[n + "_jpg"].tobytes())
        H, W = (int(v) for v in n.split("_")[0].split("x"))
        assert images.image_size(p) == (H, W, 3)
    prog = str(tmp_path / "prog.jpeg")
    with open(prog, "wb") as f:
        f.write(g19["17x23_420_prog_jpg"].tobytes())
    with pytest.raises(RuntimeError, match="PIL"):
        images.image_size(prog)
    monkeypatch.undo()
    try:
        import PIL  # noqa: F401
    except ImportError:
        return
    assert images.image_size(prog) == (17, 23, 3)


def test_decode_entry_refuses_bad_arguments_without_a_gpu():
    from swnerf import _lib
    L = _lib.lib()
    assert L.swnerf_jpeg_coef_count(17, 23, 3, _lib.JPEG_420) == 64 * (4 * 4 + 2 * 4) and L.swnerf_jpeg_coef_count(1, 1, 1, _lib.JPEG_444) == 64
    assert L.swnerf_jpeg_coef_count(65535, 65535, 3, _lib.JPEG_444) == 64 * 3 * 8192 * 8192 and L.swnerf_jpeg_coef_count(65536, 1, 3, 0) == 0
    assert L.swnerf_jpeg_coef_count(8, 8, 1, _lib.JPEG_420) == 0 and L.swnerf_jpeg_coef_count(8, 8, 2, 0) == 0
    assert L.swnerf_jpeg_decode(None, None, 0, 8, 8, 3, _lib.JPEG_420, 3, None, None, None) == 0     # n == 0: a successful no-op
    for args in ((1, 8, 8, 3, 0, 3), (1, 0, 8, 3, 0, 3), (1, 8, 65536, 3, 0, 3), (1, 8, 8, 2, 0, 3), (1, 8, 8, 3, 3, 3), (1, 8, 8, 3, 0, 5),
                 (-1, 8, 8, 3, 0, 3), (1, 8, 8, 1, 1, 3)):
        n, H, W, nc, s, co = args
        assert L.swnerf_jpeg_decode(None, None, n, H, W, nc, s, co, None, None, None) == _lib.E_ARG, args       # NULL pointers at the least
    assert L.swnerf_jpeg_entropy(b"\xff\xd8", 2, None, 0) == _lib.E_ARG
    data = b"\xff\xd8\xff\xe0 no picture"
    buf = np.zeros(64, np.int16)
    assert L.swnerf_jpeg_entropy(data, len(data), buf.ctypes.data, 64) == _lib.E_UNSUPP


def test_numpy_statement_equals_libjpeg_on_every_fixture(g19):
    """tests/jpeg_ref.py, which the tight-allocation tool compares the kernels with, is itself pinned to the golden pixels"""
    import jpeg_ref
    for n in _names(g19):
        if n.endswith("_prog"):
            continue
        j = _header(g19[n + "_jpg"].tobytes())
        got = jpeg_ref.decode(j.coefficients(), j.qt, j.H, j.W, j.ncomp, j.sampling)
        np.testing.assert_array_equal(got, g19[n + "_rgb"], err_msg=n)
