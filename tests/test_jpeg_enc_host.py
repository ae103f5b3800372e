"""The host half of the JPEG encode, and the whole encode restated, without a GPU.

g20_jpeg_enc.npz (tests/golden/make_golden_jpeg_enc.py) holds pixels and the files PIL - libjpeg - makes of them.
  * tests/jpeg_enc_ref.py, the numpy statement of the device arithmetic plus a Python Huffman writer, reproduces every one byte for
    byte, and live PIL output for 50 seeded random sizes when PIL imports;
  * tests/jpeg_enc_host_main.cpp - a stand-alone program that loops the lane functions the two kernels consist of
    (csrc/jpeg_enc_math.h) over std::vectors that end where the data ends and then runs the writer (csrc/jpeg_enc_host.h) - is
    built with g++ under AddressSanitizer and UBSan (a plain build only when the sanitizer link itself fails; the program prints
    which build ran) and must give the same bytes, on the fixtures and on the sizes the tight-allocation tool runs on the GPU;
  * swnerf_jpeg_quant_tables, swnerf_jpeg_file_bound and swnerf_jpeg_write are checked through the ctypes binding, which needs no
    GPU for these calls."""
import io
import os
import subprocess
import threading

import numpy as np
import pytest

import jpeg_enc_ref as R

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CSRC = os.path.join(ROOT, "sw-nerf_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "g20_jpeg_enc.npz")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
SIZES = ["1x1", "8x8", "24x8", "17x23", "40x72", "50x35"]


@pytest.fixture(scope="module")
def g20():
    return dict(np.load(GOLDEN, allow_pickle=False))


@pytest.fixture(scope="module")
def files(g20):
    return R.golden_files(g20)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("jpeg_enc_host") / "jpeg_enc_host_main")
    base = ["g++", "-O1", "-g", "-std=c++17", "-fno-strict-aliasing", "-I", CSRC, os.path.join(ROOT, "tests", "jpeg_enc_host_main.cpp"), "-o", exe]
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


def test_fixture_set_is_the_one_the_cases_need(g20, files):
    assert len(files) == 6 * 4 * 4 * 3 + 3 + 2 + 2
    for hw in SIZES:
        for kind in ("random", "ramp", "flat"):
            for s in ("444", "422", "420", "gray"):
                for q in (8, 50, 90, 100):
                    assert f"{hw}_{kind}_{s}_q{q}" in files
    assert g20["stack_px"].shape == (3, 17, 23, 3) and g20["float_px"].dtype == np.float32 and g20["disp_px"].dtype == np.float32
    assert np.isnan(g20["float_px"]).any() and (g20["float_px"] < 0).any() and (g20["float_px"] > 1).any() and np.isnan(g20["disp_px"]).any()
    assert float(g20["disp_max"]) == float(np.nanmax(g20["disp_px"])) and g20["qt"].shape == (100, 2, 64)
    assert os.path.getsize(GOLDEN) < 400 * 1024
    assert str(g20["pil_version"]) and "jpeg" in str(g20["libjpeg_version"])


def test_numpy_statement_reproduces_every_golden_file(g20, files):
    for n, px, ncomp, s, q in R.golden_cases(g20):
        assert R.encode(px, q, R.SAMPLING_OF[s], ncomp) == files[n], n
    for k in range(3):
        assert R.encode(g20["stack_px"][k], 90, R.S420) == files[f"stack_{k}"]
    for k in range(2):
        assert R.encode(R.to8b(g20["float_px"][k]), 90, R.S420) == files[f"float_{k}"]
        assert R.encode(R.to8b(g20["disp_px"][k], g20["disp_max"]), 90, R.S420) == files[f"disp_{k}"]


def test_rows_are_replicated_after_the_down_sampling(g20):
    """padding the rows of the full-resolution planes first and averaging then gives other chroma samples wherever the last chroma
    row averages two different rows: the fixtures 8 x 8 and 50 x 35 at 4:2:0 observe the order"""
    for hw in ("8x8", "50x35"):
        px = g20[f"px_{hw}_random"]
        H = px.shape[0]
        tall = np.concatenate([px, np.repeat(px[-1:], 16 - H % 16, 0)])      # rows replicated BEFORE: one more MCU row of the last row
        cb, cb_tall = R.planes(px, 3, R.S420)[1], R.planes(tall, 3, R.S420)[1]
        rows = cb.shape[0]
        assert np.array_equal(cb[:H // 2], cb_tall[:H // 2]) and not np.array_equal(cb[H // 2:rows], cb_tall[H // 2:rows]), hw


def test_numpy_statement_reproduces_live_pil():
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(20261019)
    for k in range(50):
        H, W = (int(v) for v in rng.integers(1, 65, 2))
        q = int(rng.integers(1, 101))
        s = ("444", "422", "420", "gray")[k % 4]
        smooth = np.cumsum(rng.integers(-6, 7, (H, W, 3)), 1) + 128
        px = (rng.integers(0, 256, (H, W, 3)) if k % 3 == 0 else np.clip(smooth, 0, 255)).astype(np.uint8)
        buf = io.BytesIO()
        if s == "gray":
            Image.fromarray(px[..., 1].copy(), "L").save(buf, format="JPEG", quality=q)
            got = R.encode(px[..., 1], q, R.S444, 1)
        else:
            Image.fromarray(px, "RGB").save(buf, format="JPEG", quality=q, subsampling={"444": 0, "422": 1, "420": 2}[s])
            got = R.encode(px, q, R.SAMPLING_OF[s], 3)
        assert got == buf.getvalue(), (H, W, q, s)


def _line(d, name, px, divisor, ncomp, s, q, want):
    """one line of the program's list: the pixels ([n,H,W,c]) and the expected bytes (n files, one after another) go to files"""
    px = np.ascontiguousarray(px)
    with open(os.path.join(d, name + ".px"), "wb") as f:
        f.write(px.tobytes())
    with open(os.path.join(d, name + ".jpg"), "wb") as f:
        f.write(want)
    kind = "u8" if px.dtype == np.uint8 else "f32"
    return f"{os.path.join(d, name + '.px')} {px.shape[1]} {px.shape[2]} {px.shape[3]} {kind} {float(divisor)!r} {ncomp} {R.SAMPLING_OF[s]} {q} {os.path.join(d, name + '.jpg')}"


def test_host_program_reproduces_every_golden_file(program, g20, files, tmp_path):
    d = str(tmp_path)
    lines = []
    for n, px, ncomp, s, q in R.golden_cases(g20):
        lines.append(_line(d, n, px[None, ..., None] if px.ndim == 2 else px[None], 0, ncomp, s, q, files[n]))
    rgba = np.concatenate([g20["px_17x23_random"], np.full((17, 23, 1), 7, np.uint8)], -1)
    lines.append(_line(d, "rgba", rgba[None], 0, 3, "420", 90, files["17x23_random_420_q90"]))
    gray3 = g20["px_40x72_ramp"][None, ..., 1:2]                              # one input channel, three components: R = G = B
    lines.append(_line(d, "gray3", gray3, 0, 3, "420", 50, R.encode(gray3[0], 50, R.S420, 3)))
    lines.append(_line(d, "stack", g20["stack_px"], 0, 3, "420", 90, b"".join(files[f"stack_{k}"] for k in range(3))))
    lines.append(_line(d, "float", g20["float_px"], 0, 3, "420", 90, files["float_0"] + files["float_1"]))
    lines.append(_line(d, "disp", g20["disp_px"][..., None], float(g20["disp_max"]), 3, "420", 90, files["disp_0"] + files["disp_1"]))
    with open(tmp_path / "list.txt", "w") as f:
        f.write("\n".join(lines) + "\n")
    r = _run(program, "check", str(tmp_path / "list.txt"))
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert r.stdout.count(": equal ") == len(lines) and "MISMATCH" not in r.stdout and "REFUSED" not in r.stdout and "0 bad" in r.stdout


def test_host_program_on_the_sizes_of_the_tight_allocation_tool(program, tmp_path):
    d = str(tmp_path)
    lines = []
    for name, px, s in R.tight_cases():
        u8 = px if px.dtype == np.uint8 else R.to8b(px)
        lines.append(_line(d, name, px, 0, 3, s, 90, b"".join(R.encode(u8[k], 90, R.SAMPLING_OF[s]) for k in range(2))))
    with open(tmp_path / "list.txt", "w") as f:
        f.write("\n".join(lines) + "\n")
    r = _run(program, "check", str(tmp_path / "list.txt"))
    assert r.returncode == 0 and r.stdout.count(": equal ") == len(lines) == 24 and "0 bad" in r.stdout, r.stdout[-4000:] + r.stderr[-2000:]


# ---- the ctypes binding ---------------------------------------------------------------------------------------------------
def _tables(quality):
    from swnerf import _lib
    qt = np.zeros((2, 64), np.uint16)
    assert _lib.lib().swnerf_jpeg_quant_tables(quality, qt.ctypes.data) == 0
    return qt


def _write(coef, qt, H, W, ncomp, sampling, cap):
    from swnerf import _lib
    out = np.full((cap + 64,), 0xA5, np.uint8)                              # 64 guard bytes behind the capacity
    n = _lib.lib().swnerf_jpeg_write(coef.ctypes.data, coef.size, qt.ctypes.data, H, W, ncomp, sampling, out.ctypes.data, cap)
    assert (out[cap:] == 0xA5).all()
    return n, out[:max(n, 0)].tobytes()


def test_quant_tables_equal_pil_at_every_quality(g20):
    for q in range(1, 101):
        np.testing.assert_array_equal(_tables(q), g20["qt"][q - 1], err_msg=str(q))
        np.testing.assert_array_equal(R.quant_tables(q), g20["qt"][q - 1], err_msg=str(q))
    np.testing.assert_array_equal(_tables(0), g20["qt"][0])                  # clipped to 1..100
    np.testing.assert_array_equal(_tables(-5), g20["qt"][0])
    np.testing.assert_array_equal(_tables(1000), g20["qt"][99])
    assert (_tables(100) == 1).all() and _tables(1).max() == 255 and _tables(50)[0, :3].tolist() == [16, 11, 10]


def test_file_bound_holds_for_every_fixture(g20, files):
    from swnerf import _lib
    L = _lib.lib()
    for n, px, ncomp, s, q in R.golden_cases(g20):
        bound = L.swnerf_jpeg_file_bound(px.shape[0], px.shape[1], ncomp, R.SAMPLING_OF[s])
        assert bound >= len(files[n]) and bound == (625 if ncomp == 3 else 330) + 2 + 416 * R.coef_count(px.shape[0], px.shape[1], ncomp, R.SAMPLING_OF[s]) // 64, n
    assert L.swnerf_jpeg_file_bound(0, 8, 3, 0) == 0 and L.swnerf_jpeg_file_bound(8, 8, 1, _lib.JPEG_420) == 0 and L.swnerf_jpeg_file_bound(8, 65536, 3, 0) == 0
    # the worst block the writer accepts: every AC coefficient at 10 bits with the longest codes does not pass the bound
    coef = np.tile(np.array([1023, -1023], np.int16), 32 * 6)
    coef[::64] = [1023, -1024, 1023, -1024, 1023, -1024]
    n, data = _write(coef, _tables(100), 16, 16, 3, _lib.JPEG_420, L.swnerf_jpeg_file_bound(16, 16, 3, _lib.JPEG_420))
    assert n > 0 and n == len(data) and data[-2:] == b"\xff\xd9"


def test_writer_equals_golden_and_refuses_short_buffers(g20, files):
    from swnerf import _lib
    L = _lib.lib()
    for n, px, ncomp, s, q in R.golden_cases(g20):
        if not (n.endswith("_q90") or n.startswith("50x35")):
            continue
        H, W = px.shape[:2]
        sampling = R.SAMPLING_OF[s]
        qt = _tables(q)
        coef = R.coefficients(px, qt, ncomp, sampling)
        want = files[n]
        size, data = _write(coef, qt, H, W, ncomp, sampling, L.swnerf_jpeg_file_bound(H, W, ncomp, sampling))
        assert size == len(want) and data == want, n
        assert _write(coef, qt, H, W, ncomp, sampling, len(want)) == (len(want), want), n                  # the exact size is enough
        for cap in (0, 1, 19, 20, 300, 624, len(want) // 2, len(want) - 2, len(want) - 1):
            assert _write(coef, qt, H, W, ncomp, sampling, min(cap, len(want) - 1))[0] == _lib.E_ARG, (n, cap)
        assert b"does not fit" in L.swnerf_last_error()
    coef, qt = np.zeros(64, np.int16), _tables(90)
    out = np.zeros(4096, np.uint8)
    assert L.swnerf_jpeg_write(coef.ctypes.data, 63, qt.ctypes.data, 8, 8, 1, 0, out.ctypes.data, 4096) == _lib.E_ARG         # the wrong count
    assert L.swnerf_jpeg_write(None, 64, qt.ctypes.data, 8, 8, 1, 0, out.ctypes.data, 4096) == _lib.E_ARG
    assert L.swnerf_jpeg_write(coef.ctypes.data, 64, qt.ctypes.data, 8, 8, 1, 0, out.ctypes.data, -1) == _lib.E_ARG
    assert L.swnerf_jpeg_write(coef.ctypes.data, 64, qt.ctypes.data, 8, 8, 2, 0, out.ctypes.data, 4096) == _lib.E_ARG
    bad = qt.copy()
    bad[0, 5] = 256
    assert L.swnerf_jpeg_write(coef.ctypes.data, 64, bad.ctypes.data, 8, 8, 1, 0, out.ctypes.data, 4096) == _lib.E_ARG          # a 16-bit table entry
    coef[1] = 1024                                                                                                              # an AC value of 11 bits
    assert L.swnerf_jpeg_write(coef.ctypes.data, 64, qt.ctypes.data, 8, 8, 1, 0, out.ctypes.data, 4096) == _lib.E_DATA
    coef[:2] = [2047, 0]
    assert L.swnerf_jpeg_write(coef.ctypes.data, 64, qt.ctypes.data, 8, 8, 1, 0, out.ctypes.data, 4096) > 0
    coef[0] = 2048                                                                                                              # a DC difference of 12 bits
    assert L.swnerf_jpeg_write(coef.ctypes.data, 64, qt.ctypes.data, 8, 8, 1, 0, out.ctypes.data, 4096) == _lib.E_DATA


def test_written_files_decode_with_the_native_reader(g20, files):
    """swnerf_jpeg_entropy of a written file gives the coefficients back, and the header its geometry and tables"""
    from swnerf import images
    for n, px, ncomp, s, q in R.golden_cases(g20):
        if not n.endswith("random_" + s + "_q50"):
            continue
        qt = _tables(q)
        coef = R.coefficients(px, qt, ncomp, R.SAMPLING_OF[s])
        j = images._jpeg_header(files[n], n)
        assert (j.H, j.W, j.ncomp, j.sampling) == (px.shape[0], px.shape[1], ncomp, R.SAMPLING_OF[s]), n
        np.testing.assert_array_equal(j.qt.reshape(ncomp, 64), qt[[0, 1, 1][:ncomp]], err_msg=n)
        np.testing.assert_array_equal(j.coefficients(), coef, err_msg=n)


def test_writer_from_several_threads(g20, files):
    from swnerf import _lib
    px, qt = g20["px_40x72_random"], _tables(90)
    coef = R.coefficients(px, qt, 3, R.S420)
    bound = _lib.lib().swnerf_jpeg_file_bound(40, 72, 3, R.S420)
    got = [None] * 6

    def work(k):
        got[k] = [_write(coef, qt, 40, 72, 3, R.S420, bound)[1] for _ in range(20)]
    threads = [threading.Thread(target=work, args=(k,)) for k in range(6)]
    [t.start() for t in threads]
    [t.join() for t in threads]
    assert all(d == files["40x72_random_420_q90"] for ds in got for d in ds)


def test_encode_entry_refuses_bad_arguments_without_a_gpu():
    from swnerf import _lib
    L = _lib.lib()
    assert L.swnerf_jpeg_encode(None, 1, 0, 8, 8, 3, 0.0, None, 3, _lib.JPEG_420, None, None, None) == 0       # n == 0: a successful no-op
    for args in ((1, 8, 8, 3, 3, 0), (1, 0, 8, 3, 3, 0), (1, 8, 65536, 3, 3, 0), (1, 8, 8, 2, 3, 0), (1, 8, 8, 5, 3, 0), (1, 8, 8, 3, 2, 0),
                 (1, 8, 8, 3, 3, 3), (1, 8, 8, 3, 1, 0), (1, 8, 8, 1, 1, 1), (-1, 8, 8, 3, 3, 0)):
        n, H, W, cin, nc, s = args
        assert L.swnerf_jpeg_encode(None, 1, n, H, W, cin, 0.0, None, nc, s, None, None, None) == _lib.E_ARG, args    # NULL pointers at the least
