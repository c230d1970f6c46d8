"""Scene editing on the device: the edit engine of the reference's GUI (gui.py; gui_obj.py is the same engine) without Tk.

The reference uploads every frame as fp32 (albedo, shading repeated to three channels, residual, two int64 maps: 52 bytes
per pixel) and, on every slider tick, runs ``update_img`` (gui.py:139-182): per semantic class a boolean-mask gather and a
scatter, then four elementwise kernels and a blocking ``.cpu()``.  Here a frame is classified ONCE - ``inerf_edit_frame``
(csrc/edit.hip) searches the nearest anchor as ``dest_class`` does and leaves, per pixel, the global row of its centre (its
*slot*, -1 where the pixel keeps its albedo) - and every later tick is one streaming launch of ``inerf_edit_recompose[_u8]``
over 7 source bytes, the slot and 3 output bytes per pixel; a whole recorded sequence is re-edited in one launch.

``EditSession`` speaks the reference's vocabulary:

=====================================================  =====================================================================
gui.py                                                 here
=====================================================  =====================================================================
``load_all_image`` + ``cluster_img`` (:185-281, :529)  ``add_frames_u8`` (the PNG bytes as they are) / ``add_pack`` / ``from_refresh``
``update_color`` (:49-60)                              ``set_color(semantic_idx, class_idx, red, green, blue)``
``scale_shading`` / ``scale_residual`` (:478-488)      ``shading_scale`` / ``residual_scale``
``f_shading`` / ``f_residual`` (:490-514)              ``change_shading`` / ``change_residual``
``reset_rgb_center`` (:337-352)                        ``reset()``
``get_cluster_num`` (:322-335)                         ``pick(i, y, x)``
``update_img`` (:139-182)                              ``frame(i)`` / ``sequence()``; a render of this package: ``edit_render(maps)``
``save_cluster_config`` (:313-320)                     ``save(dir)``
=====================================================  =====================================================================

There is no CPU path: a session on a host device raises.
"""
import bisect

import numpy as np
import torch

from . import cluster, frames, kernels
from .refresh import ClusterRefresh


# ---- host logic (no device) ------------------------------------------------------------------------------------------------------
def center_ranges(clusters):
    """``center_begin`` of ``cluster.ClusterTables`` on the host: class c owns rows ``begin[c] .. begin[c + 1]`` of the centre
    table (an empty range for a class without a cluster)."""
    begin = [0]
    for c in clusters:
        begin.append(begin[-1] + (int(torch.as_tensor(cluster._field(c, "rgb_centers")).reshape(-1, 3).shape[0]) if cluster._has(c) else 0))
    return begin


def slot_to_class(center_begin, slot):
    """``(semantic_idx, class_idx)`` of a slot - the global row of a centre; None for -1 (a pixel without a cluster)."""
    slot = int(slot)
    if slot == -1:
        return None
    if not 0 <= slot < center_begin[-1]:
        raise ValueError(f"slot {slot} lies outside the {center_begin[-1]} centres")
    sem = bisect.bisect_right(center_begin, slot) - 1          # the last class whose range begins at or before the slot
    return sem, slot - center_begin[sem]


def class_to_slot(center_begin, semantic_idx, class_idx):
    """The global centre row of ``rgb_centers[semantic_idx][class_idx]``."""
    sem, cls = int(semantic_idx), int(class_idx)
    if not 0 <= sem < len(center_begin) - 1:
        raise ValueError(f"semantic_idx {semantic_idx} lies outside the {len(center_begin) - 1} classes")
    count = center_begin[sem + 1] - center_begin[sem]
    if count == 0:
        raise ValueError(f"semantic class {sem} has no cluster (rgb_centers[{sem}] is None)")
    if not 0 <= cls < count:
        raise ValueError(f"class_idx {class_idx} lies outside the {count} centres of semantic class {sem}")
    return center_begin[sem] + cls


def slider_color(red, green, blue):
    """``float(v) / 255.0`` of the three sliders (gui.py:54-60), each 0 ... 255."""
    out = []
    for name, v in (("red", red), ("green", green), ("blue", blue)):
        v = float(v)
        if not 0.0 <= v <= 255.0:
            raise ValueError(f"{name}={v} lies outside 0 ... 255")
        out.append(v / 255.0)
    return tuple(out)


def check_frames_u8(albedo, shading, residual, label):
    """The arrays ``load_all_image`` holds before its division (gui.py:216-237), as uint8: albedo [F, H, W, 3], shading
    [F, H, W], residual [F, H, W, 3] and label [F, H, W] (or [F, H, W, 1]; integers; None: every pixel is class 0).  Returns
    them as contiguous numpy arrays and ``(F, H, W)``."""
    def host(x):
        return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    albedo, shading, residual = host(albedo), host(shading), host(residual)
    for name, a in (("albedo", albedo), ("shading", shading), ("residual", residual)):
        if a.dtype != np.uint8:
            raise ValueError(f"{name} must be uint8 (the PNG bytes, before the division by 255), got {a.dtype}")
    if albedo.ndim != 4 or albedo.shape[3] != 3:
        raise ValueError(f"albedo has shape {albedo.shape}, expected [F, H, W, 3]")
    F, H, W = albedo.shape[:3]
    if shading.shape == (F, H, W, 1):
        shading = shading[..., 0]
    if shading.shape != (F, H, W) or residual.shape != (F, H, W, 3):
        raise ValueError(f"shading {shading.shape} / residual {residual.shape} do not match albedo {albedo.shape}")
    if label is not None:
        label = host(label)
        if label.shape == (F, H, W, 1):
            label = label[..., 0]
        if label.shape != (F, H, W) or label.dtype.kind not in "iu":
            raise ValueError(f"label must hold integers of shape {(F, H, W)}, got {label.dtype} {label.shape}")
        if label.size and (int(label.min()) < -(1 << 24) or int(label.max()) > (1 << 24)):
            raise ValueError("label values beyond 2^24 are not exact in the fp32 label column")
        label = np.ascontiguousarray(label)
    return np.ascontiguousarray(albedo), np.ascontiguousarray(shading), np.ascontiguousarray(residual), label, (F, H, W)


class _Block:
    """Frames that one launch re-edits: a u8 sequence (back to back in three planes) or one fp32 pack."""

    def __init__(self, kind, n_frames, shape, **fields):
        self.kind, self.n_frames, self.shape = kind, n_frames, shape
        self.slot = None
        self.__dict__.update(fields)


class EditSession:
    """``manager``: anything ``cluster.tables_for`` accepts - this package's ``Cluster_Manager`` (one loaded from a
    ``clusters.json`` directory included) or the reference's.  ``centers`` stays the original table; ``edit_centers`` is the
    device copy the kernels read and ``set_color`` writes."""

    def __init__(self, manager, device=None):
        device = torch.device("cuda" if device is None else device)
        if device.type != "cuda":
            raise RuntimeError(f"EditSession on {device}: intrinsicnerf_amd runs only on a HIP device (no CPU / eager fallback exists)")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self.device, self.manager = device, manager
        self.clusters = list(manager.clusters)[:manager.class_num]             # as cluster.dest_class
        self.center_begin = center_ranges(self.clusters)
        self.tables = cluster.tables_for(manager, self.clusters, device)
        self.centers = self.tables.centers
        self.edit_centers = self.centers.clone()
        self._host_centers = self.centers.cpu().numpy().copy()      # pick's colours: one slot read per pick, no second copy
        self._blocks, self._frames = [], []                       # frame i -> (block, index inside the block)
        self._streamers = {}
        self.shading_scale = self.residual_scale = 1.0
        self.change_shading = self.change_residual = False

    # ---- sources ----------------------------------------------------------------------------------------------------------------
    def add_frames_u8(self, albedo, shading, residual, label=None):
        """``load_all_image``'s arrays before the division (``check_frames_u8``).  Every frame is classified once (``cluster_img``,
        gui.py:268-281) from a transient fp32 pack of ``u8 / 255``; the session keeps the three u8 planes and the slots - 11 bytes
        per pixel.  Returns the index of the first frame added."""
        albedo, shading, residual, label, (F, H, W) = check_frames_u8(albedo, shading, residual, label)
        n, dev = H * W, self.device
        a = torch.from_numpy(albedo).to(dev).reshape(F * n, 3)
        s = torch.from_numpy(shading).to(dev).reshape(F * n)
        r = torch.from_numpy(residual).to(dev).reshape(F * n, 3)
        labelled = label is not None
        slot = torch.empty(F * n, dtype=torch.int32, device=dev)
        # (v / 255.).astype(float32) of all 256 values, as numpy rounds them (gui.py:218): the pack is a gather from it
        lut = torch.from_numpy((np.arange(256) / 255.).astype(np.float32)).to(dev)
        with torch.cuda.device(dev):
            for f in range(F):
                rows = slice(f * n, (f + 1) * n)
                pack = torch.empty(n, 8, dtype=torch.float32, device=dev)
                pack[:, 0:3] = lut[a[rows].long()]
                pack[:, 3] = lut[s[rows].long()]
                pack[:, 4:7] = lut[r[rows].long()]
                pack[:, 7] = torch.from_numpy(label[f].reshape(n).astype(np.float32)).to(dev) if labelled else 0.0
                _, _, got = kernels.edit_frame(self.tables, self.edit_centers, pack, 0, 3, 4, 7 if labelled else -1, want_c=False, want_slot=True)
                slot[rows] = got
        first = len(self._frames)
        block = _Block("u8", F, (H, W), albedo=a, shading=s, residual=r)
        block.slot = slot
        self._blocks.append(block)
        self._frames += [(block, f) for f in range(F)]
        return first

    def add_pack(self, pack, widths, keys, shape=None):
        """One frame as the fp32 pack a ``render_path`` already holds on the device ([n, sum(widths)], ``frames.pack_maps``): kept as
        it is, its slots cached on first use.  A ``sem_label*`` map is the label column; without one every pixel belongs to
        class 0.  ``shape``: (H, W) of the returned images ([n, 3] without).  Returns the frame's index."""
        labelled = any(k.startswith("sem_label") for k in keys)
        return self._add_pack_cols(pack, ClusterRefresh._columns(widths, keys, labelled), shape)

    def _add_pack_cols(self, pack, cols, shape):
        pack = kernels._dev(pack, "pack", (None, None))
        if pack.device != self.device:
            raise ValueError(f"pack is on {pack.device}, the session on {self.device}")
        shape = (pack.shape[0],) if shape is None else tuple(int(v) for v in shape)
        if int(np.prod(shape)) != pack.shape[0]:
            raise ValueError(f"shape {shape} does not hold the pack's {pack.shape[0]} pixels")
        block = _Block("pack", 1, shape, pack=pack, cols=dict(cols))
        self._blocks.append(block)
        self._frames.append((block, 0))
        return len(self._frames) - 1

    @classmethod
    def from_refresh(cls, refresh):
        """A session on the manager a ``ClusterRefresh`` just fitted and the device packs it still holds (``finish`` done, ``snap``
        not yet run for them): frame indices follow the refresh's."""
        if refresh.tables is None or not refresh._kept:
            raise RuntimeError("EditSession.from_refresh: the refresh holds no fitted manager or no device packs (finish() first; snap() releases them)")
        session = cls(refresh.manager, refresh.device)
        for i in sorted(refresh._kept):
            session._add_pack_cols(refresh._kept[i], refresh._cols[i], (refresh.H, refresh.W))
        return session

    @property
    def n_frames(self):
        return len(self._frames)

    # ---- state ------------------------------------------------------------------------------------------------------------------
    def set_color(self, semantic_idx, class_idx, red, green, blue):
        """``update_color`` (gui.py:49-60): ``rgb_centers[semantic_idx][class_idx] = float(v) / 255.0`` - one 12-byte device write."""
        row = class_to_slot(self.center_begin, semantic_idx, class_idx)
        value = torch.tensor(slider_color(red, green, blue), dtype=torch.float32)      # the fp32 tensor assignment's rounding
        self.edit_centers[row].copy_(value)
        self._host_centers[row] = value.numpy()

    def reset(self):
        """``reset_rgb_center`` (gui.py:337-352): the original centres, both scales 1, both transfers off."""
        self.edit_centers.copy_(self.centers)
        self._host_centers = self.centers.cpu().numpy().copy()
        self.shading_scale = self.residual_scale = 1.0
        self.change_shading = self.change_residual = False

    def pick(self, i, y, x):
        """``get_cluster_num`` (gui.py:322-335): ``(semantic_idx, class_idx, (r, g, b))`` of pixel (y, x) of frame ``i`` - its
        centre's current colour - from one slot read; None for a pixel without a cluster."""
        block, f = self._frame(i)
        if len(block.shape) != 2:
            raise ValueError("pick needs a frame with an (H, W) shape")
        H, W = block.shape
        y, x = int(y), int(x)
        if not (0 <= y < H and 0 <= x < W):
            raise ValueError(f"pixel ({y}, {x}) lies outside the {H} x {W} frame")
        hit = slot_to_class(self.center_begin, int(self._slots(block)[f * H * W + y * W + x]))
        if hit is None:
            return None
        return hit[0], hit[1], tuple(float(v) for v in self._host_centers[self.center_begin[hit[0]] + hit[1]])

    def save(self, cluster_manager_dir):
        """``save_cluster_config`` (gui.py:313-320): the manager with the edited centres, in the reference's ``clusters.json`` /
        ``c<i>/config.json`` format.  The session's own manager is left as it was."""
        edited = self.edit_centers.cpu()
        out = cluster.Cluster_Manager(class_num=self.manager.class_num, device="cpu")
        for k, c in enumerate(list(self.manager.clusters)):
            if c is None or k >= len(self.clusters) or not cluster._has(c):
                out.clusters.append(None)
                continue
            copy = cluster.Cluster(device="cpu", intensity_factor=cluster._field(c, "intensity_factor"))
            batch = cluster._field(c, "batch_size")
            copy.batch_size = copy.batch_size if batch is None else batch
            copy.anchors = torch.as_tensor(cluster._field(c, "anchors")).detach().cpu()
            copy.links = torch.as_tensor(cluster._field(c, "links")).detach().cpu()
            copy.rgb_centers = edited[self.center_begin[k]:self.center_begin[k + 1]].clone()
            out.clusters.append(copy)
        out.save(cluster_manager_dir)
        return out

    # ---- output -----------------------------------------------------------------------------------------------------------------
    def _frame(self, i):
        i = int(i)
        if not 0 <= i < len(self._frames):
            raise IndexError(f"frame {i} of {len(self._frames)}")
        return self._frames[i]

    def _state(self):
        return dict(shading_mode=int(bool(self.change_shading)), residual_mode=int(bool(self.change_residual)),
                    shading_scale=float(self.shading_scale), residual_scale=float(self.residual_scale))

    def _slots(self, block):
        if block.slot is None:                              # a pack seen for the first time: the search form, slots kept
            c = block.cols
            _, _, block.slot = kernels.edit_frame(self.tables, self.edit_centers, block.pack, c["albedo"], c["shading"], c["residual"], c["label"],
                                                  want_c=False, want_slot=True)
        return block.slot

    def _launch(self, block, first, count, c_albedo):
        """One launch over frames ``first .. first + count`` of a block; the output buffer of ``kernels.edit_*``."""
        with torch.cuda.device(self.device):
            if block.kind == "pack":
                c = block.cols
                if block.slot is None:
                    out, _, block.slot = kernels.edit_frame(self.tables, self.edit_centers, block.pack, c["albedo"], c["shading"], c["residual"],
                                                            c["label"], want_c=c_albedo, want_slot=True, **self._state())
                else:
                    out, _ = kernels.edit_recompose(self.tables, self.edit_centers, block.pack, c["albedo"], c["shading"], c["residual"],
                                                    block.slot, want_c=c_albedo, **self._state())
                return out
            n = block.shape[0] * block.shape[1]
            rows = slice(first * n, (first + count) * n)
            out, _ = kernels.edit_recompose_u8(self.tables, self.edit_centers, block.albedo[rows], block.shading[rows], block.residual[rows],
                                               block.slot[rows], want_c=c_albedo, **self._state())
            return out

    def _streamer(self, shape):
        if shape not in self._streamers:
            self._streamers[shape] = frames.FrameStreamer(self.device)
        self._streamers[shape].drain()                      # what an abandoned sequence() left in flight
        return self._streamers[shape]

    @staticmethod
    def _images(host, n, shape, c_albedo):
        """The [.., 3] uint8 images inside a fetched output buffer: ``result``, or ``(c, result)`` with ``c_albedo``."""
        result = host[-1, :3 * n].reshape(*shape, 3)
        return (host[0, :3 * n].reshape(*shape, 3), result) if c_albedo else result

    def frame(self, i, c_albedo=False):
        """``update_img(i)`` (gui.py:139-182): the edited frame ``to8b(img)`` as an [H, W, 3] uint8 host array; with ``c_albedo`` the
        pair ``(to8b(cluster_albedo), to8b(img))`` - view mode 1 and view mode 0."""
        block, f = self._frame(i)
        out = self._launch(block, f, 1, c_albedo)
        streamer = self._streamer(tuple(out.shape))
        streamer.push(out)
        return self._images(streamer.pop(), int(np.prod(block.shape)), block.shape, c_albedo)

    def sequence(self, c_albedo=False):
        """Every resident frame under the current edit, in order: ONE launch per u8 sequence (and one per pack), the frames copied
        to the host one behind the other while the caller works on the one before."""
        for block in self._blocks:
            n = int(np.prod(block.shape))
            out = self._launch(block, 0, block.n_frames, c_albedo)
            views = [out[:, 3 * n * f:3 * n * (f + 1)] if block.n_frames > 1 else out for f in range(block.n_frames)]
            streamer = self._streamer(tuple(views[0].shape))
            streamer.push(views[0])
            for f in range(block.n_frames):
                if f + 1 < block.n_frames:
                    streamer.push(views[f + 1])
                yield self._images(streamer.pop(), n, block.shape, c_albedo)

    def edit_render(self, maps, shape=None, c_albedo=False):
        """The edit of a frame this package just rendered - a novel view - through the search form, nothing kept: ``maps`` holds
        the device maps by name (object level: ``albedo_map`` / ``shading_map`` / ``residual_map``; SSR: ``albedo_fine`` ... and
        ``sem_label``); every other map is ignored.  Returns what ``frame`` returns ([n, 3] images without ``shape``)."""
        picked = {}
        for prefix, width in (("albedo", 3), ("shading", 1), ("residual", 3), ("sem_label", 1)):
            hits = [k for k in maps if k.startswith(prefix)]
            if len(hits) > 1 or (not hits and prefix != "sem_label"):
                raise ValueError(f"edit_render needs exactly one {prefix}* map; keys = {list(maps)}")
            if hits:
                picked[hits[0]] = maps[hits[0]].detach().reshape(-1, width)
        keys = list(picked)
        pack, widths = frames.pack_maps(picked, keys)
        if pack.device != self.device:
            raise RuntimeError(f"edit_render: the maps live on {pack.device}, the session on {self.device} (no CPU / eager fallback exists)")
        c = ClusterRefresh._columns(widths, keys, any(k.startswith("sem_label") for k in keys))
        n = pack.shape[0]
        shape = (n,) if shape is None else tuple(int(v) for v in shape)
        with torch.cuda.device(self.device):
            out, _, _ = kernels.edit_frame(self.tables, self.edit_centers, pack, c["albedo"], c["shading"], c["residual"], c["label"],
                                           want_c=c_albedo, **self._state())
        streamer = self._streamer(tuple(out.shape))
        streamer.push(out)
        return self._images(streamer.pop(), n, shape, c_albedo)
