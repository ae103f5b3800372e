"""swnerf.video's container step without a GPU: write_avi's file is parsed back by tests/avi_ref.py, a RIFF reader written from the
container description; the 2 GiB refusal; mimwrite's mapping of name and quality."""
import os

import numpy as np
import pytest

import avi_ref

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _frames():
    g = dict(np.load(os.path.join(ROOT, "tests", "golden", "g20_jpeg_enc.npz"), allow_pickle=False))
    import jpeg_enc_ref
    f = jpeg_enc_ref.golden_files(g)
    frames = [f[f"stack_{k}"] for k in range(3)] + [f["17x23_random_420_q8"], f["17x23_flat_420_q100"]]
    assert any(len(x) & 1 for x in frames) and any(not len(x) & 1 for x in frames)          # odd and even lengths: both paddings
    return frames


@pytest.mark.parametrize("fps", [30, 24, 29.97, 12.5])
def test_write_avi_parses_back(tmp_path, fps):
    from swnerf import video
    frames = _frames()
    path = tmp_path / "v.avi"
    assert video.write_avi(path, frames, 17, 23, fps) == str(path)
    assert os.listdir(tmp_path) == ["v.avi"]                                 # the temporary file was renamed
    data = path.read_bytes()
    o = avi_ref.parse(data)                                                  # chunk sizes and even padding are asserted in there
    assert o["frames"] == frames
    assert o["total_frames"] == o["stream_frames"] == len(frames) and o["streams"] == 1
    assert abs(o["rate"] / o["scale"] - fps) < 1e-9 and abs(o["usec_per_frame"] - 1e6 / fps) <= 0.5
    assert (o["width"], o["height"], o["bi_width"], o["bi_height"]) == (23, 17, 23, 17) and o["rect"] == (0, 0, 23, 17)
    assert o["handler"] == b"MJPG" and o["compression"] == b"MJPG" and o["bits"] == 24 and o["flags"] & 0x10
    assert len(o["index"]) == len(frames)
    for (fourcc, flags, off, size), (pos, msize), f in zip(o["index"], o["movi"], frames):
        assert fourcc == b"00dc" and flags & 0x10 and size == msize == len(f)
        assert o["movi_tag"] + off == pos and data[pos:pos + 4] == b"00dc" and data[pos + 8:pos + 8 + size] == f
    assert len(data) % 2 == 0 and len(data) == video.avi_bytes([len(f) for f in frames], len(video._headers(len(frames), 17, 23, fps, [len(f) for f in frames])))


def test_write_avi_refuses_two_gib_and_leaves_nothing(tmp_path, monkeypatch):
    from swnerf import video
    frames = _frames()
    monkeypatch.setattr(video, "avi_bytes", lambda sizes, header_len: (1 << 31))
    with pytest.raises(ValueError, match="2 GiB"):
        video.write_avi(tmp_path / "big.avi", frames, 17, 23, 30)
    assert os.listdir(tmp_path) == []
    monkeypatch.setattr(video, "avi_bytes", lambda sizes, header_len: (1 << 31) - 1)                # the largest plain AVI passes
    video.write_avi(tmp_path / "ok.avi", frames, 17, 23, 30)
    assert os.listdir(tmp_path) == ["ok.avi"]
    with pytest.raises(ValueError, match="no frames"):
        video.write_avi(tmp_path / "none.avi", [], 17, 23, 30)
    with pytest.raises(ValueError, match="fps"):
        video.write_avi(tmp_path / "none.avi", frames, 17, 23, 0)
    assert os.listdir(tmp_path) == ["ok.avi"]


def test_a_failed_write_leaves_no_temporary_file(tmp_path, monkeypatch):
    from swnerf import video

    def boom(src, dst):
        raise OSError("no rename today")
    monkeypatch.setattr(video.os, "replace", boom)
    with pytest.raises(OSError):
        video.write_avi(tmp_path / "v.avi", _frames(), 17, 23, 30)
    assert os.listdir(tmp_path) == []


def test_mimwrite_maps_name_and_quality(tmp_path, monkeypatch):
    from swnerf import video
    calls = []
    monkeypatch.setattr(video, "write_video", lambda path, frames, fps=30, quality=90, **kw: calls.append((path, np.asarray(frames).shape, fps, quality)) or path)
    ims = [np.zeros((4, 6, 3), np.uint8)] * 5
    assert video.mimwrite(str(tmp_path / "x.mp4"), ims, fps=30, quality=8) == str(tmp_path / "x.avi")
    assert video.mimwrite(str(tmp_path / "a.b" / "spiral_rgb.mp4"), np.stack(ims), fps=12, quality=10, macro_block_size=8) == str(tmp_path / "a.b" / "spiral_rgb.avi")
    video.mimwrite(str(tmp_path / "y.gif"), ims, quality=0)
    video.mimwrite(str(tmp_path / "z"), ims)
    assert calls == [(str(tmp_path / "x.avi"), (5, 4, 6, 3), 30, 90), (str(tmp_path / "a.b" / "spiral_rgb.avi"), (5, 4, 6, 3), 12, 100),
                     (str(tmp_path / "y.avi"), (5, 4, 6, 3), 30, 50), (str(tmp_path / "z.avi"), (5, 4, 6, 3), 30, 90)]
