"""A plain RIFF walker for the Motion-JPEG AVI files of ``frames.MovieWriter``: `parse(data)` checks every size and the even
alignment of every chunk and returns the headers' fields, the frame chunks and the index.  A helper: no tests inside."""
import struct


def chunks(data, start, end):
    """[(fourcc, payload start, payload length)] of the chunks in data[start:end]; every chunk starts on an even offset."""
    out, at = [], start
    while at < end:
        assert at % 2 == 0 and at + 8 <= end, f"chunk header at {at} (region ends at {end})"
        tag, size = data[at:at + 4], struct.unpack_from("<I", data, at + 4)[0]
        assert at + 8 + size <= end, f"chunk {tag!r} at {at}: {size} bytes run past {end}"
        out.append((tag, at + 8, size))
        at += 8 + size + (size & 1)
    assert at == end or at == end + 1, (at, end)
    return out


def parse(data):
    assert data[:4] == b"RIFF" and data[8:12] == b"AVI "
    riff = struct.unpack_from("<I", data, 4)[0]
    assert riff + 8 == len(data), (riff, len(data))
    top = chunks(data, 12, len(data))
    assert [t for t, _, _ in top] == [b"LIST", b"LIST", b"idx1"]
    (_, hdrl_at, hdrl_size), (_, movi_at, movi_size), (_, idx_at, idx_size) = top
    assert data[hdrl_at:hdrl_at + 4] == b"hdrl" and data[movi_at:movi_at + 4] == b"movi"
    hdrl = chunks(data, hdrl_at + 4, hdrl_at + hdrl_size)
    assert [t for t, _, _ in hdrl] == [b"avih", b"LIST"]
    out = {}
    _, at, size = hdrl[0]
    assert size == 56
    keys = ("usec_per_frame", "max_bytes_per_sec", "padding", "flags", "total_frames", "initial_frames", "streams", "buffer_size",
            "width", "height")
    out["avih"] = dict(zip(keys, struct.unpack_from("<10I", data, at)))
    _, at, size = hdrl[1]
    assert data[at:at + 4] == b"strl"
    strl = chunks(data, at + 4, at + size)
    assert [t for t, _, _ in strl] == [b"strh", b"strf"]
    _, at, size = strl[0]
    assert size == 56
    v = struct.unpack_from("<4s4sIHHIIIIIIiI4H", data, at)
    out["strh"] = dict(type=v[0], handler=v[1], flags=v[2], scale=v[6], rate=v[7], start=v[8], length=v[9], buffer_size=v[10],
                       quality=v[11], sample_size=v[12], frame=v[13:17])
    _, at, size = strl[1]
    assert size == 40
    v = struct.unpack_from("<IiiHH4sIiiII", data, at)
    out["strf"] = dict(size=v[0], width=v[1], height=v[2], planes=v[3], bit_count=v[4], compression=v[5], size_image=v[6])
    out["movi_at"] = movi_at                                     # of the 'movi' fourcc in the file
    out["frames"] = []
    for tag, at, size in chunks(data, movi_at + 4, movi_at + movi_size):
        assert tag == b"00dc"
        out["frames"].append((at - 8, data[at:at + size]))       # (the chunk's offset in the file, the JPEG)
    assert idx_size % 16 == 0
    out["index"] = [struct.unpack_from("<4sIII", data, idx_at + 16 * i) for i in range(idx_size // 16)]
    return out


def check(data, n, width, height, fps):
    """The consistency every MovieWriter file must have; returns the JPEG files."""
    info = parse(data)
    assert info["avih"]["total_frames"] == info["strh"]["length"] == len(info["frames"]) == len(info["index"]) == n
    assert info["avih"]["usec_per_frame"] == int(round(1e6 / fps))
    assert info["avih"]["flags"] & 0x10 and info["avih"]["streams"] == 1
    assert (info["avih"]["width"], info["avih"]["height"]) == (width, height) == (info["strf"]["width"], info["strf"]["height"])
    assert info["strh"]["type"] == b"vids" and info["strh"]["handler"] == b"MJPG" and info["strf"]["compression"] == b"MJPG"
    assert info["strf"]["size"] == 40 and info["strf"]["planes"] == 1
    assert abs(info["strh"]["rate"] / info["strh"]["scale"] - fps) < 1e-6 * fps
    for (tag, flags, offset, size), (at, jpeg) in zip(info["index"], info["frames"]):
        assert tag == b"00dc" and flags & 0x10 and info["movi_at"] + offset == at and size == len(jpeg)
        assert data[at:at + 4] == b"00dc"
    return [jpeg for _, jpeg in info["frames"]]
