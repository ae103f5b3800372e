"""A RIFF / AVI reader written from the container description (AVI RIFF File Reference: RIFF 'AVI ' { LIST hdrl { avih, LIST strl {
strh, strf } }, LIST movi { 00dc ... }, idx1 }) - not from swnerf.video - for the tests that parse what write_avi wrote."""
import struct


def _chunks(data, start, end):
    """[(fourcc, payload offset, payload size)] of the chunks in data[start:end); every chunk is padded to even length"""
    out, p = [], start
    while p < end:
        assert p + 8 <= end, "a chunk header runs past its list"
        fourcc, size = data[p:p + 4], struct.unpack("<I", data[p + 4:p + 8])[0]
        assert p + 8 + size <= end, (fourcc, size, "a chunk runs past its list")
        out.append((fourcc, p + 8, size))
        p += 8 + size + (size & 1)
        if size & 1:
            assert data[p - 1] == 0, "the pad byte is zero"
    assert p == end, "the chunks do not fill their list exactly"
    return out


def parse(data):
    """-> dict(frames, width, height, total_frames, stream_frames, rate, scale, usec_per_frame, handler, compression, bits, flags,
    index = [(fourcc, flags, offset from the 'movi' tag, size)], movi = [(absolute offset of the chunk header, size)])"""
    assert data[:4] == b"RIFF" and data[8:12] == b"AVI " and struct.unpack("<I", data[4:8])[0] == len(data) - 8
    top = _chunks(data, 12, len(data))
    assert [c[0] for c in top] == [b"LIST", b"LIST", b"idx1"]
    o = {}
    (_, hp, hs), (_, mp, ms), (_, ip, isz) = top
    assert data[hp:hp + 4] == b"hdrl" and data[mp:mp + 4] == b"movi"
    hdrl = _chunks(data, hp + 4, hp + hs)
    assert [c[0] for c in hdrl] == [b"avih", b"LIST"] and hdrl[0][2] == 56
    avih = struct.unpack("<14I", data[hdrl[0][1]:hdrl[0][1] + 56])
    o.update(usec_per_frame=avih[0], flags=avih[3], total_frames=avih[4], streams=avih[6], width=avih[8], height=avih[9])
    sp, ss = hdrl[1][1], hdrl[1][2]
    assert data[sp:sp + 4] == b"strl"
    strl = _chunks(data, sp + 4, sp + ss)
    assert [c[0] for c in strl] == [b"strh", b"strf"] and strl[0][2] == 56 and strl[1][2] == 40
    strh = data[strl[0][1]:strl[0][1] + 56]
    assert strh[:4] == b"vids"
    o["handler"] = strh[4:8]
    o["scale"], o["rate"], _, o["stream_frames"] = struct.unpack("<4I", strh[20:36])
    o["rect"] = struct.unpack("<4H", strh[48:56])
    bi = struct.unpack("<IiiHH4sIiiII", data[strl[1][1]:strl[1][1] + 40])
    assert bi[0] == 40 and bi[3] == 1
    o.update(bi_width=bi[1], bi_height=bi[2], bits=bi[4], compression=bi[5])
    movi = _chunks(data, mp + 4, mp + ms)
    assert all(c[0] == b"00dc" for c in movi)
    o["movi"] = [(p - 8, s) for _, p, s in movi]
    o["movi_tag"] = mp
    o["frames"] = [data[p:p + s] for _, p, s in movi]
    assert isz % 16 == 0
    o["index"] = [struct.unpack("<4sIII", data[ip + 16 * k:ip + 16 * k + 16]) for k in range(isz // 16)]
    return o
