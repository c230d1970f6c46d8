"""The cluster-refresh pass of ``render_path(update_cluster=True)`` on the device (run_nerf.py:142-272 | trainer.py:1221-1443).

Every 10 000 steps both reference trainers render every training view, take every second pixel of every albedo frame (and
its label) as the sample set, fit the albedo clusters on it and send every albedo frame through ``dest_color`` to write
``c###.png`` and the re-composed ``edit###.png``.  The render, the lookup and the fit have HIP paths; ``ClusterRefresh`` is
the pass that ties them together without a host round trip:

* ``add_frame`` - where a frame's pack is complete on the render stream, ``inerf_frame_subsample`` writes its share of the
  sample table (whose size is known up front) and counts its labels per class; the device pack is kept for the post-pass;
* ``finish`` - ``cluster.update_center`` on the device-resident table and labels; the K class counts are the one host read;
* ``snap`` - ``inerf_cluster_snap_compose`` turns a kept pack into the two 8-bit images, which travel to the host as one
  pinned asynchronous copy while the next frame's launch runs (``frames.FrameStreamer``).

``object_level.render_path(..., refresh=ClusterRefresh())`` and ``SSRRenderer.cluster_refresh = ClusterRefresh()`` drive it;
returned values and files are those of the host path.  There is no CPU path.
"""
import numpy as np
import torch

from . import cluster, frames, kernels


class ClusterRefresh:
    """One object per ``render_path`` front-end; reusable: ``begin`` starts a new pass.

    ``manager_factory(class_num=...)`` builds the manager that ``finish`` fits and returns; ``keep_bytes`` bounds the device
    packs held between ``add_frame`` and ``snap`` (frames beyond it are uploaded again from the caller's host arrays);
    ``step``: every step-th pixel in both directions is a sample (2 in both reference trainers)."""

    def __init__(self, manager_factory=cluster.Cluster_Manager, keep_bytes=4 << 30, step=2):
        self.manager_factory = manager_factory
        self.keep_bytes = int(keep_bytes)
        self.step = int(step)
        if self.step < 1:
            raise ValueError("step must be at least 1")
        self.manager = None
        self._reset()

    def _reset(self):
        self.pixels = self.labels = self.counts = self.tables = None
        self._kept, self._cols, self._held = {}, {}, 0
        self._streamer, self._launched, self._next, self._host = None, 0, 0, None

    def begin(self, n_frames, H, W, n_classes, device):
        """Allocates the sample table [n_frames * ceil(H / step) * ceil(W / step), 3] and, for ``n_classes`` > 1, its labels and
        the zeroed per-class counts.  With one class every pixel belongs to it and no label column is read (cluster.py:55-59)."""
        self._reset()
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError(f"ClusterRefresh on {device}: intrinsicnerf_amd runs only on a HIP device (no CPU / eager fallback exists)")
        self.device = device
        self.n_frames, self.H, self.W, self.n_classes = int(n_frames), int(H), int(W), int(n_classes)
        self.rows = -(-self.H // self.step) * -(-self.W // self.step)
        self.pixels = torch.empty(self.n_frames * self.rows, 3, dtype=torch.float32, device=device)
        if self.n_classes > 1:
            self.labels = torch.empty(self.n_frames * self.rows, dtype=torch.int64, device=device)
            self.counts = torch.zeros(self.n_classes, dtype=torch.int32, device=device)
        self._added = set()

    @staticmethod
    def _columns(widths, keys, labelled):
        """Column offsets of the albedo, shading, residual (and label) maps inside a pack."""
        at, c = {}, 0
        for k, w in zip(keys, widths):
            at[k] = (c, w)
            c += w

        def find(prefix, width):
            hits = [k for k in keys if k.startswith(prefix)]
            if len(hits) != 1 or at[hits[0]][1] != width:
                raise ValueError(f"the pack needs exactly one {prefix}* map of {width} column(s); keys = {list(keys)}")
            return at[hits[0]][0]
        return {"albedo": find("albedo", 3), "shading": find("shading", 1), "residual": find("residual", 3),
                "label": find("sem_label", 1) if labelled else -1}

    def add_frame(self, i, pack, widths, keys):
        """Frame ``i``'s pack ([H * W, sum(widths)] fp32 on the device, ``frames.pack_maps``) is complete on the current stream:
        its samples go into the table at rows ``i * rows ..``; the pack is kept for ``snap`` while the budget lasts."""
        if self.pixels is None:
            raise RuntimeError("ClusterRefresh.add_frame before begin")
        i = int(i)
        if not 0 <= i < self.n_frames or i in self._added:
            raise ValueError(f"frame {i} of {self.n_frames}: out of range or added twice")
        cols = self._columns(widths, keys, self.labels is not None)
        kernels.frame_subsample(pack, self.H, self.W, cols["albedo"], self.pixels, offset=i * self.rows, label_col=cols["label"],
                                out_labels=self.labels, class_counts=self.counts, step=self.step)
        self._added.add(i)
        size = pack.numel() * pack.element_size()
        if self._held + size <= self.keep_bytes:
            self._kept[i], self._cols[i] = pack, cols
            self._held += size

    def keeps_all(self, n_frames, pack_bytes):
        """True when ``add_frame`` will keep the pack of every one of ``n_frames`` frames of ``pack_bytes`` bytes each for ``snap`` -
        its own budget rule, counted from ``begin``: ``finish`` then needs no ``host`` arrays."""
        return self._held + int(n_frames) * int(pack_bytes) <= self.keep_bytes

    def finish(self, b_f, host=None):
        """Builds the manager (``manager_factory(class_num=n_classes)``), fits it on the table and returns it.  ``host(i)`` ->
        ``(albedo [H, W, 3], label [H, W] or None, shading [H, W], residual [H, W, 3])`` numpy arrays of frame ``i``: read by
        ``snap`` for the frames whose device pack was not kept."""
        if self.pixels is None or len(self._added) != self.n_frames:
            raise RuntimeError(f"ClusterRefresh.finish: {0 if self.pixels is None else len(self._added)} of "
                               f"{getattr(self, 'n_frames', 0)} frames were added")
        self._host = host
        manager = self.manager_factory(class_num=self.n_classes)
        with torch.cuda.device(self.device):
            # (the counts' .cpu() inside is the pass's one device->host read before the images)
            cluster.update_center(manager, self.labels, self.pixels, band_factor=b_f, counts=self.counts)
        single = self.n_classes == 1
        clusters = list(manager.clusters)[:1] if single else list(manager.clusters)[:self.n_classes]       # as cluster.dest_color
        self.tables = cluster.tables_for(manager, clusters, self.device)
        self.manager = manager
        self.pixels = self.labels = None                   # the table has served: release it before the post-pass
        return manager

    def _launch(self, i):
        n = self.H * self.W
        pack, cols = self._kept.pop(i, None), self._cols.pop(i, None)
        if pack is None:                                    # beyond the budget: one compact upload of what the kernel reads
            if self._host is None:
                raise RuntimeError(f"ClusterRefresh.snap({i}): the frame's pack was not kept (keep_bytes={self.keep_bytes}) and finish() got no host arrays")
            albedo, label, shading, residual = self._host(i)
            parts = [np.asarray(albedo, np.float32).reshape(n, 3), np.asarray(shading, np.float32).reshape(n, 1),
                     np.asarray(residual, np.float32).reshape(n, 3)]
            cols = {"albedo": 0, "shading": 3, "residual": 4, "label": -1}
            if self.n_classes > 1:
                parts.append(np.asarray(label).reshape(n, 1).astype(np.float32))          # < 2^24: exact
                cols["label"] = 7
            pack = torch.from_numpy(np.concatenate(parts, 1)).to(self.device, non_blocking=False)
        else:
            self._held -= pack.numel() * pack.element_size()
        with torch.cuda.device(self.device):
            out, _ = kernels.cluster_snap_compose(self.tables, pack, cols["albedo"], cols["shading"], cols["residual"], cols["label"])
            self._streamer.push(out)

    def snap(self, i):
        """``(c, edit)`` of frame ``i`` as [H, W, 3] uint8 host arrays: ``to8b(dest_color(albedo))`` and
        ``to8b(dest_color(albedo) * shading + residual)``.  Frames are asked for in order, 0 .. n_frames - 1; frame ``i + 1`` is
        launched before frame ``i``'s copy is waited for."""
        if self.tables is None:
            raise RuntimeError("ClusterRefresh.snap before finish")
        if self._streamer is None:
            self._streamer = frames.FrameStreamer(self.device)
        if i != self._next:
            raise ValueError(f"ClusterRefresh.snap({i}): frames are taken in order, frame {self._next} is next")
        while self._launched <= min(i + 1, self.n_frames - 1):
            self._launch(self._launched)
            self._launched += 1
        self._next += 1
        c, edit = kernels.snap_images(self._streamer.pop(), self.H * self.W)
        return c.reshape(self.H, self.W, 3), edit.reshape(self.H, self.W, 3)
