"""Image-level loop around the render path: N poses -> N frames of maps on the host.

The reference's loops (``render_path``: object_level/run_nerf.py:142-212, SSR/training/trainer.py:1221-1389) render one
image, then pull each map to the host with its own ``.cpu().numpy()`` - six blocking device->host copies per image, each
of which first waits for the whole render.  Here a frame's maps are packed into ONE device tensor, copied into one of two
pinned host buffers on a side stream, and the next frame's kernels are enqueued while that copy runs; the host touches a
frame only when the frame after it has been enqueued.  ``to8b`` happens on the device when only 8-bit images are wanted
(``inerf_frame_to_u8``), a quarter of the bytes; ``FrameProducts`` (opt-in) makes every 8- and 16-bit image of the loops - the
16-bit casts, the label colours, the (acc > 10) mask and the jet maps of ``depth2rgb`` included - in one launch per frame
(``inerf_frame_products``), and with ``FrameProducts(encode=True)`` those planes become complete PNG files on the device too
(``inerf_png_encode``, csrc/png.hip) - the host only writes bytes.  The ray batch of a pose comes from ``inerf_gen_rays`` (``inerf_gen_rays_ndc`` for NDC frames).
"""
import os
import struct
import zlib

import numpy as np
import torch

from . import kernels


class FrameStreamer:
    """Double-buffered device->host transfer of per-frame packs.

    ``push(pack)`` enqueues the copy of a device tensor (any dtype; every call must use the same shape / dtype) on a side
    stream and returns the numpy array of the frame pushed BEFORE the previous one, if it is done - frames come out in
    order, two calls late; ``drain()`` returns the rest.  The caller's stream never waits for a copy."""

    def __init__(self, device, depth=2):
        self.device = torch.device(device)
        self.copy_stream = torch.cuda.Stream(device=self.device)
        self.depth = depth
        self.slots = []          # [host buffer, event, device tensor kept alive until the copy is done]
        self.pending = []        # slot indices in flight, oldest first
        self.next = 0

    def _collect(self, slot):
        host, event, _ = self.slots[slot]
        event.synchronize()
        self.slots[slot][2] = None
        return host.numpy().copy()

    def push(self, pack):
        out = None
        free = [s for s in range(len(self.slots)) if s not in self.pending]      # slots emptied by pop()
        if free:
            slot = free[0]
        elif len(self.slots) < self.depth:
            self.slots.append([torch.empty(pack.shape, dtype=pack.dtype, pin_memory=True), torch.cuda.Event(), None])
            slot = len(self.slots) - 1
        else:
            slot = self.pending.pop(0)
            out = self._collect(slot)
        host = self.slots[slot][0]
        if host.shape != pack.shape or host.dtype != pack.dtype:
            raise ValueError("FrameStreamer: every frame must have the same shape and dtype")
        ready = torch.cuda.Event()
        ready.record(torch.cuda.current_stream(self.device))       # the pack is complete on the render stream here
        with torch.cuda.stream(self.copy_stream):
            self.copy_stream.wait_event(ready)
            host.copy_(pack, non_blocking=True)
            self.slots[slot][1].record(self.copy_stream)
        self.slots[slot][2] = pack                                  # keep the device tensor alive until then
        self.pending.append(slot)
        return out

    def pop(self):
        """The oldest frame in flight (waits for its copy alone); None when nothing is in flight.  With ``depth`` >= 2 a caller
        that pushes frame i + 1 before it pops frame i works on a frame while the next one is computed and copied."""
        return self._collect(self.pending.pop(0)) if self.pending else None

    def drain(self):
        out = [self._collect(s) for s in self.pending]
        self.pending = []
        return out


def pack_maps(maps, keys):
    """[n, sum(widths)] fp32 tensor of the named per-ray maps side by side (one copy instead of len(keys))."""
    cols = [maps[k].reshape(maps[k].shape[0], -1).float() for k in keys]
    return torch.cat(cols, 1), [c.shape[1] for c in cols]


def unpack_frame(frame, widths, keys, image_shape):
    out, c = {}, 0
    for k, w in zip(keys, widths):
        a = frame[:, c:c + w]
        out[k] = a.reshape(*image_shape, w) if w > 1 else a.reshape(*image_shape)
        c += w
    return out


def write_png(path, image):
    """Minimal PNG encoder (8-bit grey / RGB, 16-bit grey) for hosts without imageio - the reference writes its frames
    with ``imageio.imwrite`` (run_nerf.py:193-211), which is used instead when importable."""
    a = np.ascontiguousarray(image)
    if a.dtype != np.uint16:          # 16-bit maps (disp / depth in mm, trainer.py:1359,1365: format="png", prefer_uint8=False) always
        try:                          # take the encoder below: what imageio does with uint16 depends on its version and plugin
            import imageio
            if hasattr(imageio, "imwrite"):
                imageio.imwrite(path, image)
                return
        except ImportError:
            pass
    if a.dtype == np.uint16:
        depth, a = 16, a.astype(">u2")
    elif a.dtype == np.uint8:
        depth = 8
    else:
        raise ValueError(f"write_png: dtype {a.dtype}")
    if a.ndim == 2:
        colour, h, w = 0, *a.shape
    elif a.ndim == 3 and a.shape[2] == 3:
        colour, (h, w) = 2, a.shape[:2]
    else:
        raise ValueError(f"write_png: shape {a.shape}")
    raw = b"".join(b"\x00" + a[r].tobytes() for r in range(h))

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xffffffff)

    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, colour, 0, 0, 0))
                + chunk(b"IDAT", zlib.compress(raw, 6)) + chunk(b"IEND", b""))


def encode_png(image, filter=None):
    """The PNG file (``bytes``) of a device tensor - uint8 [H, W] or [H, W, 3], uint16 [H, W] - encoded on the device
    (``inerf_png_encode``).  ``filter``: a PNG filter type 0 .. 4 for every row; default: the adaptive choice per row.  Waits for the
    file's length, then copies that many bytes."""
    if not isinstance(image, torch.Tensor):
        raise TypeError("encode_png takes a device tensor; write_png writes a numpy array")
    if not image.is_cuda:
        raise RuntimeError(f"encode_png: the image lives on {image.device}; PNG files are encoded only on a HIP device (no CPU / eager "
                           "fallback exists)")
    if image.dtype == torch.uint8 and (image.dim() == 2 or (image.dim() == 3 and image.shape[2] == 3)):
        channels, depth = (1 if image.dim() == 2 else 3), 8
    elif image.dtype == getattr(torch, "uint16", None) and image.dim() == 2:
        channels, depth = 1, 16
    else:
        raise ValueError(f"encode_png: dtype {image.dtype}, shape {tuple(image.shape)}")
    spec = (image.shape[0], image.shape[1], channels, depth, 0) + (() if filter is None else (int(filter),))
    plan = kernels.png_plan([spec])
    out, sizes = kernels.png_encode(image.contiguous().view(torch.uint8).reshape(-1), plan)
    return out[:int(sizes[0])].cpu().numpy().tobytes()


def encode_jpeg(image, quality=90):
    """The baseline JPEG file (``bytes``) of a device tensor - uint8 [H, W] (grey) or [H, W, 3] (RGB, stored as YCbCr 4:4:4) - encoded
    on the device (``inerf_jpeg_encode``) into a worst-case arena.  Waits for the file's length, then copies that many bytes."""
    if not isinstance(image, torch.Tensor):
        raise TypeError("encode_jpeg takes a device tensor")
    if not image.is_cuda:
        raise RuntimeError(f"encode_jpeg: the image lives on {image.device}; JPEG files are encoded only on a HIP device (no CPU / eager "
                           "fallback exists)")
    if not (image.dtype == torch.uint8 and (image.dim() == 2 or (image.dim() == 3 and image.shape[2] == 3))):
        raise ValueError(f"encode_jpeg: dtype {image.dtype}, shape {tuple(image.shape)}")
    h, w, c = int(image.shape[0]), int(image.shape[1]), 1 if image.dim() == 2 else 3
    stream = kernels.JpegStream(h, w, c, quality, kernels.jpeg_frame_bound(h, w, c), 1, image.device)
    kernels.jpeg_encode(image.contiguous().reshape(-1), kernels.jpeg_plan([(h, w, c, quality, 0)]), [stream])
    state = stream.state.cpu().numpy()          # cursor (2), status, index
    if state[2] != 0 or state[1] != 1:
        raise RuntimeError(f"encode_jpeg: the frame was refused (status {int(state[2])}) by an arena of {stream.capacity} bytes")
    return stream.arena[8:8 + int(state[4])].cpu().numpy().tobytes()


def _avi_chunk(tag, data):
    return tag + struct.pack("<I", len(data)) + data + (b"\0" if len(data) & 1 else b"")


def avi_head(entries, movi_bytes, width, height, fps):
    """``(head, idx1)`` of a Motion-JPEG AVI file whose ``LIST movi`` payload is ``movi_bytes`` long and holds the chunks
    ``entries`` = [(offset in the payload, JPEG length)]: the file is ``head + payload + idx1``.  ``RIFF 'AVI '``, ``LIST hdrl``
    with ``avih`` and one ``strl`` (``strh``: vids / MJPG; ``strf``: a BITMAPINFOHEADER with biCompression 'MJPG'), ``LIST movi``,
    then ``idx1`` with one keyframe entry per frame, offsets counted from the ``movi`` fourcc.  4 GiB or more: ValueError (OpenDML
    is not written)."""
    from fractions import Fraction
    n = len(entries)
    rate = Fraction(fps).limit_denominator(1000000)
    if rate <= 0:
        raise ValueError(f"fps = {fps}")
    usec = int(round(1e6 / float(fps)))
    biggest = max([size for _, size in entries], default=0)
    avih = struct.pack("<14I", usec, int(biggest * float(fps)) & 0xffffffff, 0, 0x10, n, 0, 1, biggest, width, height, 0, 0, 0, 0)
    strh = b"vidsMJPG" + struct.pack("<IHHIIIIIIiI4H", 0, 0, 0, 0, rate.denominator, rate.numerator, 0, n, biggest, -1, 0, 0, 0, width, height)
    strf = struct.pack("<IiiHH4sIiiII", 40, width, height, 1, 24, b"MJPG", width * height * 3, 0, 0, 0, 0)
    strl = b"LIST" + struct.pack("<I", 4 + 8 + len(strh) + 8 + len(strf)) + b"strl" + _avi_chunk(b"strh", strh) + _avi_chunk(b"strf", strf)
    hdrl = b"LIST" + struct.pack("<I", 4 + 8 + len(avih) + len(strl)) + b"hdrl" + _avi_chunk(b"avih", avih) + strl
    idx1 = _avi_chunk(b"idx1", b"".join(b"00dc" + struct.pack("<III", 0x10, 4 + offset, size) for offset, size in entries))
    riff = 4 + len(hdrl) + 12 + movi_bytes + len(idx1)
    if riff + 8 >= 1 << 32:
        raise ValueError(f"the AVI file would hold {riff + 8} bytes: 4 GiB or more needs OpenDML, which is not written")
    head = b"RIFF" + struct.pack("<I", riff) + b"AVI " + hdrl + b"LIST" + struct.pack("<I", 4 + movi_bytes) + b"movi"
    return head, idx1


def avi_bytes(files, width, height, fps=30):
    """The Motion-JPEG AVI file of a list of JPEG files (``bytes``) - the host side of ``MovieWriter``: each file becomes a '00dc'
    chunk exactly as the device lays it into the arena."""
    payload, entries = b"", []
    for data in files:
        entries.append((len(payload), len(data)))
        payload += _avi_chunk(b"00dc", bytes(data))
    head, idx1 = avi_head(entries, len(payload), width, height, fps)
    return head + payload + idx1


class MovieWriter:
    """A Motion-JPEG AVI file written from device frames - what ``imageio.mimwrite`` / ``cv2.VideoWriter`` do on the host at the end
    of the reference's render passes.  Owns the device arena, cursor, index and status word (``kernels.JpegStream``); ``add(plane)``
    encodes a device uint8 frame ([H, W] or [H, W, 3]) into the arena and waits for nothing; ``close()`` copies the used part of the
    arena and the index to the host once and writes the file.

    The arena holds ``frames * (header + bytes_per_sample * samples)`` bytes; ``bytes_per_sample=None`` sizes it by
    ``inerf_jpeg_frame_bound``, so it cannot overflow.  ``frames=None``: 64.  Once ``frames`` frames were added the used part goes to
    the host (one wait) and the arena is used again, so a longer movie costs one copy per ``frames`` frames.  A frame that did not fit
    sets the status word: ``close()`` then raises a RuntimeError that names the capacity it needed."""

    def __init__(self, path, shape, channels, fps=30, quality=90, frames=None, bytes_per_sample=1.0, device=None, _tail=0):
        self.path, self.fps = path, fps
        self.shape, self.channels, self.quality = (int(shape[0]), int(shape[1])), int(channels), int(quality)
        if self.channels not in (1, 3):
            raise ValueError(f"MovieWriter: {channels} channels")
        device = torch.device("cuda" if device is None else device)
        if device.type != "cuda":
            raise RuntimeError(f"MovieWriter on {device}: frames are encoded only on a HIP device (no CPU / eager fallback exists)")
        self.frames = 64 if frames is None else int(frames)
        if self.frames < 1:
            raise ValueError(f"MovieWriter: frames = {frames}")
        h, w = self.shape
        self.bound = kernels.jpeg_frame_bound(h, w, self.channels)
        header = len(kernels.jpeg_header(h, w, self.channels, self.quality))
        per_frame = self.bound if bytes_per_sample is None else header + int(float(bytes_per_sample) * h * w * self.channels)
        self.stream = kernels.JpegStream(h, w, self.channels, self.quality, self.frames * per_frame, self.frames, device, tail=_tail)
        self.plan = kernels.jpeg_plan([(h, w, self.channels, self.quality, 0)])
        self.workspace = torch.empty(max(self.plan[1], 1), dtype=torch.uint8, device=device)
        self.count, self.parts, self.entries, self.bytes, self.closed = 0, [], [], 0, False

    def _check(self, plane):
        want = self.shape + ((3,) if self.channels == 3 else ())
        if not isinstance(plane, torch.Tensor):
            raise TypeError("MovieWriter.add takes a device tensor")
        if not plane.is_cuda:
            raise RuntimeError(f"MovieWriter.add: the frame lives on {plane.device}; frames are encoded only on a HIP device (no CPU / "
                               "eager fallback exists)")
        if plane.dtype != torch.uint8 or tuple(plane.shape) != want:
            raise ValueError(f"MovieWriter.add: dtype {plane.dtype}, shape {tuple(plane.shape)}; the movie holds uint8 {want}")

    def reserve(self, n=1):
        """Room for ``n`` more index entries: when the arena's ``frames`` are used up, its used part goes to the host first."""
        if self.closed:
            raise RuntimeError("MovieWriter: closed")
        if n > self.frames:
            raise ValueError(f"{n} frames in one call; the arena was made for {self.frames}")
        if self.count + n > self.frames:
            self._flush()
        self.count += n

    def add(self, plane):
        self._check(plane)
        self.reserve(1)
        kernels.jpeg_encode(plane.contiguous().reshape(-1), self.plan, [self.stream], workspace=self.workspace)

    def _flush(self):
        state = self.stream.state.cpu().numpy()
        used, written, status = int(state[0]), int(state[1]), int(state[2])
        if status:
            raise RuntimeError(f"MovieWriter({self.path!r}): a frame did not fit the arena of {self.stream.capacity} bytes ({self.frames} "
                               f"frames); it needed a capacity of {status} bytes - raise bytes_per_sample, or pass None for the bound")
        if written != self.count:
            raise RuntimeError(f"MovieWriter({self.path!r}): {self.count} frames were added, the device wrote {written}")
        index = state[3:3 + 2 * written].reshape(-1, 2)
        self.entries += [(self.bytes + int(o), int(n)) for o, n in index]
        if used:
            self.parts.append(self.stream.arena[:used].cpu().numpy())
        self.bytes += used
        self.stream.state[:2].zero_()
        self.count = 0

    def close(self):
        """Writes the file: head, the arena's bytes verbatim as the ``movi`` payload, ``idx1``.  Returns the path."""
        if self.closed:
            return self.path
        self.closed = True
        self._flush()
        h, w = self.shape
        head, idx1 = avi_head(self.entries, self.bytes, w, h, self.fps)
        with open(self.path, "wb") as f:
            f.write(head)
            for part in self.parts:
                f.write(part.tobytes())
            f.write(idx1)
        self.parts = []
        return self.path


def write_movie(path, stack, fps=30, quality=90):
    """``imageio.mimwrite(path, stack, fps=..., quality=...)`` as a Motion-JPEG AVI file made on the device: ``stack`` is a numpy array
    or tensor [N, H, W] or [N, H, W, 3], uint8 (a list of equal frames is stacked); batches of up to 16 frames are uploaded and each
    batch is encoded in one ``inerf_jpeg_encode`` call into one arena.  ``quality``: JPEG quality 1 .. 100.  Returns the path."""
    if isinstance(stack, (list, tuple)):
        stack = torch.stack(list(stack)) if all(isinstance(f, torch.Tensor) for f in stack) else np.stack([np.asarray(f) for f in stack])
    if not isinstance(stack, torch.Tensor):
        stack = torch.from_numpy(np.ascontiguousarray(stack))
    if stack.dtype != torch.uint8 or not (stack.dim() == 3 or (stack.dim() == 4 and stack.shape[3] == 3)) or stack.shape[0] < 1:
        raise ValueError(f"write_movie: dtype {stack.dtype}, shape {tuple(stack.shape)}; expected uint8 [N, H, W] or [N, H, W, 3]")
    n, h, w = (int(v) for v in stack.shape[:3])
    c = 1 if stack.dim() == 3 else 3
    device = stack.device if stack.is_cuda else torch.device("cuda", torch.cuda.current_device())
    batch = min(n, kernels._capi.JPEG_MAX_IMAGES)
    writer = MovieWriter(path, (h, w), c, fps=fps, quality=quality, frames=batch, bytes_per_sample=None, device=device)
    plane = h * w * c
    plans = {}
    workspace = None
    for start in range(0, n, batch):
        count = min(batch, n - start)
        src = stack[start:start + count].to(device).contiguous().reshape(-1)
        if count not in plans:
            plans[count] = kernels.jpeg_plan([(h, w, c, quality, k * plane) for k in range(count)])
        writer.reserve(count)
        workspace = kernels.jpeg_encode(src, plans[count], [writer.stream] * count, workspace=workspace)
    return writer.close()


def to8b(x):
    """(255 * clip(x, 0, 1)).astype(uint8) - run_nerf_helpers.py:13: numpy arrays on the host, device tensors through
    ``inerf_frame_to_u8``."""
    if isinstance(x, torch.Tensor):
        return kernels.frame_to_u8(x.float().contiguous()) if x.is_cuda else (255 * torch.clamp(x, 0, 1)).to(torch.uint8)
    return (255 * np.clip(x, 0, 1)).astype(np.uint8)


class FrameProducts:
    """The 8- and 16-bit images of a render_path loop, made on the device from each frame's pack (csrc/frame_vis.hip): one
    ``inerf_frame_products`` launch per frame, preceded by one ``inerf_frame_range`` per jet product that colours a map by its
    own range; the bytes travel through a ``FrameStreamer`` of their own.  Opt-in; both front-ends read one
    (``ssr.SSRRenderMixin.frame_products``, ``object_level.render_path(products=...)``) and hand it their product list.

    A product is ``(name, kind, key[, parameter])`` over the pack's ``keys``:
      ``(name, "to8b", key)``            uint8, [H, W] or [H, W, 3] with the map's width: ``to8b``
      ``(name, "u16", key, scale)``      uint16 [H, W]: ``(map * scale).astype(np.uint16)``
      ``(name, "u8_cast", key)``         uint8 [H, W]: ``map.astype(np.uint8)``
      ``(name, "thresh", key, t)``       uint8 [H, W]: ``to8b(float32(map > t))``
      ``(name, "palette", key)``         uint8 [H, W, 3]: ``palette[map]``, black outside the palette
      ``(name, "jet", key, (lo, hi))``   uint8 [H, W, 3]: ``depth2rgb(map, lo, hi)``; ``None`` instead of the pair: the map's own range

    ``encode=True``: every plane is also encoded to a PNG file on the device (``inerf_png_encode``: three more launches per frame,
    adaptive row filter, one dynamic-Huffman block per 32 KiB segment); the files travel through a second ``FrameStreamer`` in their
    worst-case buffers, with their lengths behind them, and ``files(i)`` hands out ``{name: bytes}``.  ``images(i)`` is unchanged.

    ``movies={product_name: path}`` (with ``fps=`` and ``quality=``): every frame's plane of each named product is also appended to
    a Motion-JPEG AVI file (``MovieWriter``) - one ``inerf_jpeg_encode`` call per frame for all of them, after the products launch;
    ``close_movies()`` writes the files (the front-ends' ``render_path`` calls it after the last pose).  A ``u16`` product cannot be
    a movie.
    """

    KINDS = {name: k for k, name in enumerate(kernels._capi.FRAME_KIND_NAMES)}

    def __init__(self, encode=False, movies=None, fps=30, quality=90):
        self.names = None
        self.encode = bool(encode)
        self.movies, self.fps, self.quality = dict(movies or {}), fps, int(quality)
        self.writers = []

    def begin(self, products, keys, widths, image_shape, device, palette=None):
        """Starts a pass: ``products`` over a pack of ``keys`` / ``widths`` (``pack_maps``) whose rows are the pixels of an
        ``image_shape`` = (H, W) frame.  ``palette``: uint8 [C, 3] (numpy or tensor), copied to the device once."""
        capi = kernels._capi
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError(f"FrameProducts on {device}: intrinsicnerf_amd runs only on a HIP device (no CPU / eager fallback exists)")
        start, c = {}, 0
        for k, w in zip(keys, widths):
            start[k] = (c, int(w))
            c += int(w)
        self.device, self.shape, self.columns = device, (int(image_shape[0]), int(image_shape[1])), c
        self.n = self.shape[0] * self.shape[1]
        self.palette = None
        if palette is not None:
            palette = palette.detach() if isinstance(palette, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(palette))
            self.palette = palette.to(device=device, dtype=torch.uint8).reshape(-1, 3).contiguous()
        self.names, self.kinds, self.ranged, specs = [], [], [], []
        for spec in products:
            name, kind, key = spec[0], self.KINDS[spec[1]], spec[2]
            if key not in start:
                raise KeyError(f"product {name!r} reads {key!r}; the pack holds {list(keys)}")
            if name in self.names:
                raise ValueError(f"two products are called {name!r}")
            column, width = start[key]
            a = b = 0.0
            rng = None
            if kind in (capi.FRAME_U16, capi.FRAME_THRESH):
                a = float(spec[3])
            elif kind == capi.FRAME_JET:
                if len(spec) > 3 and spec[3] is not None:
                    a, b = float(spec[3][0]), float(spec[3][1])
                else:
                    rng = torch.full((2,), float("nan"), dtype=torch.float32, device=device)
                    self.ranged.append((column, rng))
            elif kind == capi.FRAME_PALETTE and self.palette is None:
                raise ValueError(f"product {name!r} is a palette gather: begin() needs the palette")
            self.names.append(name)
            self.kinds.append((kind, width))
            specs.append((kind, column, width, a, b, rng))
        self.plan = kernels.frame_products_plan(self.n, specs, 0 if self.palette is None else self.palette.shape[0])
        self.workspace = torch.empty(max(kernels.frame_range_workspace_bytes(self.n) // 4, 1), dtype=torch.float32, device=device)
        self.streamer, self.in_flight, self.host = FrameStreamer(device), [], {}
        if self.encode:
            images = []
            for (kind, width), (offset, _) in zip(self.kinds, self.plan[1]):
                rgb = kind in (capi.FRAME_PALETTE, capi.FRAME_JET) or width == 3
                images.append((self.shape[0], self.shape[1], 3 if rgb else 1, 16 if kind == capi.FRAME_U16 else 8, offset))
            self.png_plan = kernels.png_plan(images)
            self.png_workspace = torch.empty(max(self.png_plan[3], 1), dtype=torch.uint8, device=device)
            self.file_streamer, self.files_in_flight, self.host_files = FrameStreamer(device), [], {}
        if self.movies:
            self.close_movies()                     # a pass that was begun before: its files are finished first
            images = []
            for name in self.movies:
                if name not in self.names:
                    raise KeyError(f"movies names the product {name!r}; this pass makes {self.names}")
                k = self.names.index(name)
                kind, width = self.kinds[k]
                if kind == capi.FRAME_U16:
                    raise ValueError(f"movies names the product {name!r}: a 16-bit plane cannot be a JPEG frame")
                rgb = kind in (capi.FRAME_PALETTE, capi.FRAME_JET) or width == 3
                images.append((self.shape[0], self.shape[1], 3 if rgb else 1, self.quality, self.plan[1][k][0]))
            self.writers = [MovieWriter(path, self.shape, im[2], fps=self.fps, quality=self.quality, device=device)
                            for path, im in zip(self.movies.values(), images)]
            self.jpeg_plan = kernels.jpeg_plan(images)
            self.jpeg_workspace = torch.empty(max(self.jpeg_plan[1], 1), dtype=torch.uint8, device=device)

    def close_movies(self):
        """Finishes the movie files of the pass (one copy of each arena's used part) and returns their paths."""
        writers, self.writers = self.writers, []
        return [w.close() for w in writers]

    def add_frame(self, i, pack):
        """Frame ``i``'s pack ([H * W, columns] fp32 on the device) is complete on the current stream: its planes are computed
        there and their copy to the host is enqueued.  Nothing waits."""
        if self.names is None:
            raise RuntimeError("FrameProducts.add_frame before begin")
        if not pack.is_cuda:
            raise RuntimeError(f"FrameProducts.add_frame: the pack lives on {pack.device}; the frame images are made only on a HIP "
                               "device (no CPU / eager fallback exists)")
        if tuple(pack.shape) != (self.n, self.columns):
            raise ValueError(f"the pack has shape {tuple(pack.shape)}, begin() was told {(self.n, self.columns)}")
        for column, rng in self.ranged:           # the map's own range, on the device: the product kernel reads it
            kernels.frame_range(pack[:, column], minmax=rng, workspace=self.workspace)
        out, _ = kernels.frame_products(pack, None, palette=self.palette, plan=self.plan)
        done = self.streamer.push(out)
        self.in_flight.append(int(i))
        if done is not None:
            self.host[self.in_flight.pop(0)] = done
        if self.encode:
            # the files in their worst-case places and, behind them, their lengths: one buffer, one copy
            total, count = self.png_plan[2], len(self.names)
            buf = torch.empty(total + 8 * max(count, 1), dtype=torch.uint8, device=self.device)
            kernels.png_encode(out[:self.plan[2]], self.png_plan, out=buf[:total], sizes=buf[total:].view(torch.int64),
                               workspace=self.png_workspace)
            done = self.file_streamer.push(buf)
            self.files_in_flight.append(int(i))
            if done is not None:
                self.host_files[self.files_in_flight.pop(0)] = done
        if self.writers:
            for w in self.writers:
                w.reserve(1)
            kernels.jpeg_encode(out[:self.plan[2]], self.jpeg_plan, [w.stream for w in self.writers], workspace=self.jpeg_workspace)

    def files(self, i):
        """``{name: bytes}`` of frame ``i``: each product's complete PNG file (``encode=True``).  Waits for the copies up to frame ``i``
        alone; a frame is handed out once."""
        if not self.encode:
            raise RuntimeError("FrameProducts.files: made without encode=True")
        i = int(i)
        while i not in self.host_files:
            if not self.files_in_flight:
                raise KeyError(f"FrameProducts.files({i}): no such frame in flight")
            self.host_files[self.files_in_flight.pop(0)] = self.file_streamer.pop()
        buf = self.host_files.pop(i)
        total = self.png_plan[2]
        sizes = buf[total:total + 8 * len(self.names)].view(np.int64)
        out = {}
        for name, (offset, capacity), size in zip(self.names, self.png_plan[1], sizes):
            if not 0 < size <= capacity:
                raise RuntimeError(f"FrameProducts.files({i}): {name!r} reports {int(size)} bytes, its buffer holds {capacity}")
            out[name] = buf[offset:offset + int(size)].tobytes()
        return out

    def images(self, i):
        """``{name: array}`` of frame ``i``: views of the frame's host bytes - uint8 [H, W] / [H, W, 3], uint16 [H, W].  Waits for
        the copies up to frame ``i`` alone; a frame is handed out once."""
        i = int(i)
        while i not in self.host:
            if not self.in_flight:
                raise KeyError(f"FrameProducts.images({i}): no such frame in flight")
            self.host[self.in_flight.pop(0)] = self.streamer.pop()
        buf = self.host.pop(i)
        capi, out = kernels._capi, {}
        for name, (kind, width), (offset, size) in zip(self.names, self.kinds, self.plan[1]):
            plane = buf[offset:offset + size]
            if kind == capi.FRAME_U16:
                out[name] = plane.view("<u2").reshape(self.shape)
            elif kind in (capi.FRAME_PALETTE, capi.FRAME_JET) or width == 3:
                out[name] = plane.reshape(*self.shape, 3)
            else:
                out[name] = plane.reshape(self.shape)
        return out


def depth2rgb(depth, min_value=None, max_value=None):
    """``imgviz.depth2rgb(depth, min_value=None, max_value=None)`` without imgviz or matplotlib: the jet colour map of
    ``(depth - lo) / (hi - lo)``, black where that is NaN; ``lo`` / ``hi`` default to the map's nanmin / nanmax.  fp32 throughout,
    the rule of include/inerf.h (JET).  A device tensor goes through ``inerf_frame_range`` / ``inerf_frame_products`` and comes
    back as a uint8 device tensor ``[..., 3]``; a host array through the same rule in numpy with the library's table."""
    if isinstance(depth, torch.Tensor) and depth.is_cuda:
        flat = depth.detach().float().reshape(-1, 1)
        if min_value is None or max_value is None:
            rng = kernels.frame_range(flat[:, 0])
            if min_value is not None:
                rng[0] = float(min_value)
            if max_value is not None:
                rng[1] = float(max_value)
            spec = (kernels._capi.FRAME_JET, 0, 1, 0.0, 0.0, rng)
        else:
            spec = (kernels._capi.FRAME_JET, 0, 1, float(min_value), float(max_value), None)
        out, planes = kernels.frame_products(flat, [spec])
        return out[planes[0][0]:planes[0][0] + planes[0][1]].reshape(*depth.shape, 3)
    x = np.asarray(depth.detach().numpy() if isinstance(depth, torch.Tensor) else depth, dtype=np.float32)
    import warnings
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)          # (an all-NaN map: its range is NaN and the image black)
        lo = np.float32(np.nanmin(x) if min_value is None else min_value) if x.size else np.float32("nan")
        hi = np.float32(np.nanmax(x) if max_value is None else max_value) if x.size else np.float32("nan")
        t = (x - lo) / (hi - lo)
        nan = np.isnan(t)
        c = np.minimum(np.maximum(np.where(nan, np.float32(0), t), np.float32(0)), np.float32(1))
        rgb = kernels.jet_table()[np.minimum((c * np.float32(256)).astype(np.int32), 255)]
    rgb[nan] = 0
    return rgb


def ensure_dir(path):
    if path is not None:
        os.makedirs(path, exist_ok=True)
