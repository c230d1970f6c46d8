"""Scene editing on the device (csrc/edit.hip, intrinsicnerf_amd/editing.py): inerf_edit_frame, inerf_edit_recompose and
inerf_edit_recompose_u8 against the pinned inerf_cluster_snap_compose (the un-edited case), against the reference's
``update_img`` restated in torch on the CPU (_editing.update_img: exact outside the sine mode, within a derived bound of its fp64
evaluation inside it), the cached forms against the search form, and ``EditSession`` against the same restatement step by step.

Sizes of the cached form, next to the kernel's constants (csrc/edit.hip): kGroup = 8 pixels per lane of the vector path, a
byte-path head of (out_result & 3) <= 3 pixels in front of the groups and a tail of < 8 behind them, 256 lanes = 2048 pixels
per block - so RECOMPOSE_SIZES sits either side of 8 and 2048 for every head (n, n + 1 .. n + 3 pixels in front), of a head that
swallows the frame (n <= 3), and holds a count of a few thousand."""
import ctypes as C
from functools import lru_cache

import numpy as np
import pytest
import torch

import _editing as E
from conftest import load_golden
from test_cluster import Manager, fixture_clusters

pytestmark = pytest.mark.gpu

SIZES = (1, 7, 8, 9, 16384, 16385)                                  # the 8-pixel tile's edges and the small-batch switch
RECOMPOSE_SIZES = (1, 2, 3, 4, 7, 8, 9, 11, 12, 16, 19, 2047, 2048, 2051, 2059, 4099)
GUARD = 0xA5


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


@pytest.fixture(scope="module")
def lookup_tables():
    from intrinsicnerf_amd import cluster as ic
    fx = load_golden("cluster_lookup")
    dev = _dev()
    clusters = fixture_clusters(fx, dev)
    assert len(clusters) == 5 and clusters[3] is None               # one class has no cluster
    multi = ic.ClusterTables(clusters, dev)
    assert tuple(multi.center_begin.tolist()) == E.CENTER_BEGIN
    return {"multi": multi, "single": ic.ClusterTables([clusters[4]], dev), "clusters": clusters}


def _tables(lookup_tables, mode):
    return lookup_tables["single" if mode == "ignore" else "multi"]


def _centres(tables):
    """rgb_centers as the reference's list: one [c, 3] CPU tensor per class, None without a cluster."""
    begin, ctr = tables.center_begin.tolist(), tables.centers.cpu()
    return [ctr[begin[k]:begin[k + 1]].clone() if begin[k + 1] > begin[k] else None for k in range(tables.n_classes)]


def _recoloured(tables, mode):
    """(rgb_centers list, edit_centers device table) with E.RECOLOUR applied as update_color does (gui.py:58-60)."""
    centres = _centres(tables)
    todo = E.RECOLOUR if mode != "ignore" else ((0, 4, E.RECOLOUR[2][2]), (0, 0, E.RECOLOUR[0][2]), (0, 2, E.RECOLOUR[1][2]))
    for sem, cls, (r, g, b) in todo:
        centres[sem][cls, 0] = float(r) / 255.0
        centres[sem][cls, 1] = float(g) / 255.0
        centres[sem][cls, 2] = float(b) / 255.0
    return centres, torch.cat([c for c in centres if c is not None], 0).to(tables.device).contiguous()


def _class_map(tables, pack, lab, ignore):
    """dest_class of every pixel through the pinned lookup (0 where the pixel has no cluster), on the host."""
    from intrinsicnerf_amd import cluster as ic
    dev = tables.device
    _, cls = ic.lookup(tables, pack[:, 1:4].contiguous(), None if ignore else torch.from_numpy(lab).to(dev), want_color=False,
                       want_class=True, ignore_label=ignore)
    return cls.cpu()


def _frame(tables, edit_centers, pack, ignore, **kw):
    from intrinsicnerf_amd import kernels
    return kernels.edit_frame(tables, edit_centers, pack, E.COLS["albedo"], E.COLS["shading"], E.COLS["residual"],
                              -1 if ignore else E.COLS["label"], **kw)


# ---- 1. + 2. the identity edit is the pinned kernel; slots -------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("mode", ["uniform", "random", "ignore"])
def test_identity_edit_equals_snap_compose_and_slots(lookup_tables, n, mode):
    from intrinsicnerf_amd import kernels
    dev, ignore = _dev(), mode == "ignore"
    tables = _tables(lookup_tables, mode)
    pack_np, lab = E.edit_inputs(n, mode, tables.n_classes)
    pack = torch.from_numpy(pack_np).to(dev)
    want, colour = kernels.cluster_snap_compose(tables, pack, E.COLS["albedo"], E.COLS["shading"], E.COLS["residual"],
                                                -1 if ignore else E.COLS["label"], want_color=True)
    out, result, slot = _frame(tables, tables.centers, pack, ignore, want_f32=True, want_slot=True)
    for got, ref in zip(kernels.snap_images(out, n), kernels.snap_images(want, n)):                  # (c, result) against (c, edit)
        assert torch.equal(got, ref)
    # the float colour: the centre the slot names, the albedo where it names none
    got_colour = torch.where((slot >= 0)[:, None], tables.centers[slot.clamp(min=0).long()], pack[:, 1:4])
    assert torch.equal(got_colour.view(torch.int32), colour.view(torch.int32))
    # slots: center_begin[label] + dest_class where the class has a cluster, -1 for labels -1, K, K + 1 and the empty class
    begin = tuple(tables.center_begin.tolist())
    cls = _class_map(tables, pack, lab, ignore).numpy()
    want_slot = E.expected_slots(lab, cls, begin)
    assert np.array_equal(slot.cpu().numpy(), want_slot)
    if not ignore:
        outside = (lab < 0) | (lab >= tables.n_classes) | (lab == 3)
        assert (want_slot[outside] == -1).all() and (want_slot[~outside] >= 0).all()
        if n >= 100:
            assert {-1, 3, tables.n_classes, tables.n_classes + 1} <= set(lab.tolist())
    else:
        assert (want_slot >= 0).all()
    # the float result of the identity edit: the reference's line with scales of 1 is one product and one sum
    _, img = E.update_img(pack_np[:, 1:4], pack_np[:, 0], pack_np[:, 5:8], lab, cls, _centres(tables))
    assert E.same_floats(result, img)
    # without the optional outputs nothing else changes
    out2, none_f, none_s = _frame(tables, tables.centers, pack, ignore, want_c=False)
    assert none_f is None and none_s is None and tuple(out2.shape) == (1, kernels.snap_row_bytes(n))
    assert torch.equal(out2[0, :3 * n], out[1, :3 * n])


# ---- 3. edited, non-sine modes are exact ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (8, 9, 16384, 16385))
@pytest.mark.parametrize("mode", ["uniform", "random", "ignore"])
def test_edited_frames_are_exact_outside_the_sine_mode(lookup_tables, n, mode):
    from intrinsicnerf_amd import kernels
    dev, ignore = _dev(), mode == "ignore"
    tables = _tables(lookup_tables, mode)
    pack_np, lab = E.edit_inputs(n, mode, tables.n_classes)
    pack = torch.from_numpy(pack_np).to(dev)
    cls = _class_map(tables, pack, lab, ignore)
    centres, edit_centers = _recoloured(tables, mode)
    assert not torch.equal(edit_centers, tables.centers)
    for smode in (0, 1):
        for gs, gr in E.SCALES:
            c_albedo, img = E.update_img(pack_np[:, 1:4], pack_np[:, 0], pack_np[:, 5:8], lab, cls, centres, change_shading=bool(smode),
                                         shading_scale=gs, residual_scale=gr)
            out, result, _ = _frame(tables, edit_centers, pack, ignore, shading_mode=smode, shading_scale=gs, residual_scale=gr, want_f32=True)
            assert E.same_floats(result, img), (smode, gs, gr)
            assert torch.isnan(img).any() == (n > 3)
            c, res = kernels.snap_images(out, n)
            assert np.array_equal(c.cpu().numpy(), E.to8b(c_albedo.numpy())), (smode, gs, gr)
            assert np.array_equal(res.cpu().numpy(), E.to8b(img.numpy())), (smode, gs, gr)
            want = E.to8b(img.numpy())
            assert (want[2] == 255).all() and (want[3] == 0).all()                                    # above 1, NaN
            assert (want[1] == 0).all() or smode == 1 or gs != 1.0                                    # below 0 (albedo * shading < 2)


# ---- 4. the sine mode against fp64 ---------------------------------------------------------------------------------------------------
SINE_BOUND = 4e-6          # derived, not fitted: operands up to 8 in magnitude, three individually rounded products, one sum and
#                            two roundings in the sine's argument give about 3.5e-6 over the input ranges of _editing.edit_inputs


@pytest.mark.parametrize("n", (16384, 16385))                       # one size per tile width: the share below needs a frame's worth of pixels
@pytest.mark.parametrize("mode", ["uniform", "random", "ignore"])
def test_sine_mode_against_fp64(lookup_tables, n, mode):
    from intrinsicnerf_amd import kernels
    dev, ignore = _dev(), mode == "ignore"
    tables = _tables(lookup_tables, mode)
    pack_np, lab = E.edit_inputs(n, mode, tables.n_classes)
    pack = torch.from_numpy(pack_np).to(dev)
    cls = _class_map(tables, pack, lab, ignore)
    centres, edit_centers = _recoloured(tables, mode)
    for smode in (0, 1):
        for gs, gr in E.SCALES:
            _, img = E.update_img(pack_np[:, 1:4], pack_np[:, 0], pack_np[:, 5:8], lab, cls, centres, change_shading=bool(smode),
                                  change_residual=True, shading_scale=gs, residual_scale=gr, dtype=torch.float64)
            out, result, _ = _frame(tables, edit_centers, pack, ignore, shading_mode=smode, residual_mode=1, shading_scale=gs,
                                    residual_scale=gr, want_f32=True)
            got, want = result.cpu().double(), img
            nan = torch.isnan(want)
            assert torch.equal(torch.isnan(got), nan)
            err = (got - want).abs()[~nan].max().item()
            print(f"sine mode n={n} {mode} shading_mode={smode} scales=({gs}, {gr}): max |f32 - f64| = {err:.3e}")
            assert err <= SINE_BOUND, (smode, gs, gr, err)
            # 8-bit: at most 1 off, and only where the fp64 value lies within the bound of a multiple of 1/255 (0 and 1 included)
            res = kernels.snap_images(out, n)[1].cpu().numpy().astype(np.int64)
            w = np.where(nan.numpy(), 0.0, want.numpy())
            want8 = E.to8b(w).astype(np.int64)
            near = (np.abs(w * 255.0 - np.round(w * 255.0)) <= SINE_BOUND * 255.0) & (w >= -SINE_BOUND) & (w <= 1.0 + SINE_BOUND)
            diff = np.abs(res - want8)
            assert (diff <= 1).all() and (diff[~near] == 0).all(), (smode, gs, gr)
            share = near.mean()
            print(f"    values within the bound of a multiple of 1/255: {100 * share:.3f} %, differing: {int((diff > 0).sum())}")
            assert share <= 0.005, (smode, gs, gr, share)


# ---- 5. the cached forms equal the search form ---------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def _shared_tables():
    from intrinsicnerf_amd import cluster as ic
    dev = _dev()
    tables = ic.ClusterTables(fixture_clusters(load_golden("cluster_lookup"), dev), dev)
    return tables, _recoloured(tables, "random")[1]


@lru_cache(maxsize=None)
def _search_reference(n, smode, rmode):
    """(u8 planes, labels, fp32 pack of u8 / 255, slots, c, result, float result) of the search form on a recoloured table - computed
    once per size and mode, shared, never written."""
    from intrinsicnerf_amd import kernels
    dev = _dev()
    tables, edit_centers = _shared_tables()
    albedo, shading, residual, lab = E.u8_inputs(n, tables.n_classes)
    pack = torch.from_numpy(E.u8_pack(albedo, shading, residual, lab)).to(dev)
    out, result, slot = _frame(tables, edit_centers, pack, False, shading_mode=smode, residual_mode=rmode, shading_scale=0.37,
                               residual_scale=1.63, want_f32=True, want_slot=True)
    c, res = kernels.snap_images(out, n)
    return dict(tables=tables, edit_centers=edit_centers, u8=(albedo, shading, residual), pack=pack, slot=slot, c=c.clone(), result=res.clone(),
                f32=result, state=dict(shading_mode=smode, residual_mode=rmode, shading_scale=0.37, residual_scale=1.63))


def _offset_view(host, offset, dev):
    """A device copy of a host uint8 array whose first byte sits ``offset`` bytes past an aligned allocation."""
    flat = torch.from_numpy(np.ascontiguousarray(host).reshape(-1))
    buf = torch.zeros(flat.numel() + 8, dtype=torch.uint8, device=dev)
    assert buf.data_ptr() % 16 == 0
    buf[offset:offset + flat.numel()] = flat.to(dev)
    view = buf[offset:offset + flat.numel()].view(host.shape)
    assert view.data_ptr() % 4 == offset % 4 and view.is_contiguous()
    return view


def _guarded_out(n, rows, offset, dev):
    """(whole buffer, the [rows, snap_row_bytes(n)] output view ``offset`` bytes past a 16-byte guard)."""
    from intrinsicnerf_amd import kernels
    row = kernels.snap_row_bytes(n)
    whole = torch.full((16 + offset + rows * row + 16,), GUARD, dtype=torch.uint8, device=dev)
    assert whole.data_ptr() % 16 == 0
    return whole, whole[16 + offset:16 + offset + rows * row].view(rows, row)


def _guards_untouched(whole, n, rows, offset):
    from intrinsicnerf_amd import kernels
    row = kernels.snap_row_bytes(n)
    w = whole.cpu().numpy()
    keep = np.ones(w.shape[0], bool)
    for r in range(rows):
        keep[16 + offset + r * row:16 + offset + r * row + 3 * n] = False
    return (w[keep] == GUARD).all()


@pytest.mark.parametrize("offset", (0, 1, 2, 3))
@pytest.mark.parametrize("smode,rmode", [(0, 0), (1, 1)])
def test_cached_forms_equal_the_search_form(offset, smode, rmode):
    from intrinsicnerf_amd import kernels
    dev = _dev()
    for n in RECOMPOSE_SIZES:
        ref = _search_reference(n, smode, rmode)
        tables, edit_centers, state = ref["tables"], ref["edit_centers"], ref["state"]
        # u8 form: every source and the output `offset`, `offset + 1`, `offset + 2`, `offset + 3` bytes (mod 4) off alignment
        for spread in (0, 1):
            a, s, r = (_offset_view(x, (offset + spread * (j + 1)) % 4, dev) for j, x in enumerate(ref["u8"]))
            for want_c in (True, False):
                whole, out = _guarded_out(n, 2 if want_c else 1, offset, dev)
                got, f32 = kernels.edit_recompose_u8(tables, edit_centers, a, s, r, ref["slot"], out=out, want_c=want_c, want_f32=True, **state)
                assert got.data_ptr() == out.data_ptr() and out.data_ptr() % 4 == offset
                assert torch.equal(out[-1, :3 * n].view(n, 3), ref["result"]), (n, spread, want_c)
                assert not want_c or torch.equal(out[0, :3 * n].view(n, 3), ref["c"]), (n, spread)
                assert torch.equal(f32.view(torch.int32), ref["f32"].view(torch.int32)), (n, spread, want_c)
                assert _guards_untouched(whole, n, 2 if want_c else 1, offset), (n, spread, want_c)
        # fp32 form on the same values
        whole, out = _guarded_out(n, 2, offset, dev)
        _, f32 = kernels.edit_recompose(tables, edit_centers, ref["pack"], E.COLS["albedo"], E.COLS["shading"], E.COLS["residual"], ref["slot"],
                                        out=out, want_f32=True, **state)
        assert torch.equal(out[1, :3 * n].view(n, 3), ref["result"]) and torch.equal(out[0, :3 * n].view(n, 3), ref["c"]), n
        assert torch.equal(f32.view(torch.int32), ref["f32"].view(torch.int32)) and _guards_untouched(whole, n, 2, offset), n
        # ... and without the float output
        whole, out = _guarded_out(n, 1, offset, dev)
        _, none = kernels.edit_recompose(tables, edit_centers, ref["pack"], E.COLS["albedo"], E.COLS["shading"], E.COLS["residual"], ref["slot"],
                                         out=out, want_c=False, **state)
        assert none is None and torch.equal(out[0, :3 * n].view(n, 3), ref["result"]) and _guards_untouched(whole, n, 1, offset), n


@pytest.mark.parametrize("n", (5, 19, 2051))
def test_out_c_on_its_own_alignment(n):
    """out_c and out_result at different byte alignments (the raw entry point: the launcher's buffer gives both the same one):
    out_c then leaves as bytes, out_result still as dwords."""
    from intrinsicnerf_amd import _capi
    dev = _dev()
    ref = _search_reference(n, 1, 1)
    a, s, r = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in ref["u8"])
    params = _capi.EditParams(ref["edit_centers"].data_ptr(), 1, 1, 0.37, 1.63)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    for off_r, off_c in ((0, 1), (1, 3), (2, 0), (3, 2)):
        res = torch.full((16 + off_r + 3 * n + 16,), GUARD, dtype=torch.uint8, device=dev)
        col = torch.full((16 + off_c + 3 * n + 16,), GUARD, dtype=torch.uint8, device=dev)
        rc = _capi.lib().inerf_edit_recompose_u8(C.c_void_p(a.data_ptr()), C.c_void_p(s.data_ptr()), C.c_void_p(r.data_ptr()),
                                                 C.c_void_p(ref["slot"].data_ptr()), n, C.byref(params), C.c_void_p(res.data_ptr() + 16 + off_r),
                                                 C.c_void_p(col.data_ptr() + 16 + off_c), None, stream)
        assert rc == _capi.OK
        torch.cuda.synchronize()
        for buf, off, want in ((res, off_r, ref["result"]), (col, off_c, ref["c"])):
            assert torch.equal(buf[16 + off:16 + off + 3 * n].view(n, 3), want), (off_r, off_c)
            assert (buf[:16 + off] == GUARD).all() and (buf[16 + off + 3 * n:] == GUARD).all(), (off_r, off_c)


def test_a_sequence_in_one_call_equals_frame_by_frame():
    """3 frames of 5 pixels back to back: frames 1 and 2 start 15 and 30 bytes into the planes."""
    from intrinsicnerf_amd import kernels
    dev = _dev()
    F, n = 3, 5
    ref = _search_reference(F * n, 1, 1)
    tables, edit_centers, state = ref["tables"], ref["edit_centers"], ref["state"]
    a, s, r = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in ref["u8"])
    out, f32 = kernels.edit_recompose_u8(tables, edit_centers, a, s, r, ref["slot"], want_f32=True, **state)
    c_all, res_all = kernels.snap_images(out, F * n)
    assert torch.equal(res_all, ref["result"]) and torch.equal(c_all, ref["c"])
    for f in range(F):
        rows = slice(f * n, (f + 1) * n)
        out_f, f32_f = kernels.edit_recompose_u8(tables, edit_centers, a[rows], s[rows], r[rows], ref["slot"][rows], want_f32=True, **state)
        assert a[rows].data_ptr() == a.data_ptr() + 15 * f
        c, res = kernels.snap_images(out_f, n)
        assert torch.equal(res, res_all[rows]) and torch.equal(c, c_all[rows]) and torch.equal(f32_f.view(torch.int32), f32[rows].view(torch.int32))


# ---- 6. the 8-bit conversion -----------------------------------------------------------------------------------------------------
def test_u8_conversion_is_numpys(lookup_tables):
    from intrinsicnerf_amd import kernels
    dev = _dev()
    tables = lookup_tables["multi"]
    v = np.arange(256, dtype=np.uint8)
    want = (v / 255.).astype(np.float32)
    full, zero = np.full(256, 255, np.uint8), np.zeros(256, np.uint8)
    rgb = lambda x: np.repeat(x[:, None], 3, 1)
    slot = torch.full((256,), -1, dtype=torch.int32, device=dev)
    # (albedo, shading, residual): the plane under test holds every byte value, the others 1 or 0 - result = that plane's float
    for name, (a, s, r) in (("albedo", (rgb(v), full, rgb(zero))), ("shading", (rgb(full), v, rgb(zero))), ("residual", (rgb(zero), full, rgb(v)))):
        up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
        out, f32 = kernels.edit_recompose_u8(tables, tables.centers, up(a), up(s), up(r), slot, want_f32=True)
        got = f32.cpu().numpy()
        for k in range(3):
            assert np.array_equal(got[:, k].view(np.int32), want.view(np.int32)), name
        assert np.array_equal(kernels.snap_images(out, 256)[1].cpu().numpy(), E.to8b(rgb(want))), name


# ---- 7. the session ----------------------------------------------------------------------------------------------------------------
def _session_inputs(F, H, W, K):
    n = F * H * W
    albedo, shading, residual, lab = E.u8_inputs(n, K, seed=7)
    return albedo.reshape(F, H, W, 3), shading.reshape(F, H, W), residual.reshape(F, H, W, 3), lab.reshape(F, H, W)


def test_session_follows_update_img(lookup_tables, tmp_path):
    from intrinsicnerf_amd import cluster as ic, editing, refresh
    dev = _dev()
    F, H, W = 2, 12, 16
    n = H * W
    mgr = Manager(lookup_tables["clusters"])
    albedo, shading, residual, lab = _session_inputs(F, H, W, mgr.class_num)
    session = editing.EditSession(mgr, dev)
    assert session.add_frames_u8(albedo, shading, residual, lab) == 0 and session.n_frames == F
    # the reference's startup (gui.py:529-540): dest_class of every pixel, the centres per class
    a32, s32, r32 = E.unit(albedo).reshape(F, n, 3), E.unit(shading).reshape(F, n), E.unit(residual).reshape(F, n, 3)
    flat_lab = lab.reshape(F, n)
    cls = ic.dest_class(mgr, torch.from_numpy(a32.reshape(-1, 3)).to(dev), torch.from_numpy(flat_lab.reshape(-1, 1)).to(dev)).cpu().reshape(F, n)
    centres = _centres(session.tables)
    state = dict(change_shading=False, change_residual=False, shading_scale=1.0, residual_scale=1.0)

    def want(i):
        c, img = E.update_img(a32[i], s32[i], r32[i], flat_lab[i], cls[i], centres, **state)
        return E.to8b(c.numpy()).reshape(H, W, 3), E.to8b(img.numpy()).reshape(H, W, 3)

    def check():
        for i in range(F):
            c, img = session.frame(i, c_albedo=True)
            assert c.dtype == np.uint8 and c.shape == (H, W, 3)
            assert np.array_equal(c, want(i)[0]) and np.array_equal(img, want(i)[1]) and np.array_equal(session.frame(i), want(i)[1])
        seq = list(session.sequence())
        assert len(seq) == F and all(np.array_equal(seq[i], want(i)[1]) for i in range(F))
        pairs = list(session.sequence(c_albedo=True))
        assert all(np.array_equal(pairs[i][0], want(i)[0]) and np.array_equal(pairs[i][1], want(i)[1]) for i in range(F))

    check()
    # after construction (and after reset) the frame is the refresh pass's edit image of the same data
    def snap_edit(i):
        r = refresh.ClusterRefresh()
        r.device, r.H, r.W, r.n_frames, r.n_classes, r.tables = dev, H, W, i + 1, mgr.class_num, session.tables
        for f in range(i + 1):
            pack = np.concatenate([a32[f], s32[f][:, None], r32[f], flat_lab[f][:, None].astype(np.float32)], 1)
            r._kept[f], r._cols[f] = torch.from_numpy(pack).to(dev), {"albedo": 0, "shading": 3, "residual": 4, "label": 7}
        for f in range(i + 1):
            got = r.snap(f)
        return got
    for i in range(F):
        c, edit = snap_edit(i)
        assert np.array_equal(session.frame(i), edit) and np.array_equal(session.frame(i, c_albedo=True)[0], c)
    # pick: a pixel with a cluster, one without
    begin = E.CENTER_BEGIN
    with_cluster = [(i, p) for i in range(F) for p in range(n) if 0 <= flat_lab[i, p] < 5 and flat_lab[i, p] != 3]
    without = [(i, p) for i in range(F) for p in range(n) if flat_lab[i, p] in (-1, 3, 5, 6)]
    assert with_cluster and without
    for i, p in with_cluster[:3] + with_cluster[-3:]:
        sem, k = int(flat_lab[i, p]), int(cls[i, p])
        assert session.pick(i, p // W, p % W) == (sem, k, tuple(float(v) for v in centres[sem][k]))
    for i, p in without[:3]:
        assert session.pick(i, p // W, p % W) is None
    with pytest.raises(ValueError):
        session.pick(0, H, 0)
    # set_color on the picked centre and on one of the last class, scales and transfers, step by step
    i, p = with_cluster[0]
    sem, k, _ = session.pick(i, p // W, p % W)
    for (s_, k_, (red, green, blue)) in ((sem, k, (250, 3, 99)),) + E.RECOLOUR:
        session.set_color(s_, k_, red, green, blue)
        centres[s_][k_, 0], centres[s_][k_, 1], centres[s_][k_, 2] = float(red) / 255.0, float(green) / 255.0, float(blue) / 255.0
        check()
    assert session.pick(i, p // W, p % W)[2] == tuple(float(v) for v in centres[sem][k])
    with pytest.raises(ValueError):
        session.set_color(3, 0, 1, 2, 3)                              # the class without a cluster
    for gs, gr in E.SCALES[1:]:
        session.shading_scale, session.residual_scale = gs, gr
        state.update(shading_scale=gs, residual_scale=gr)
        check()
    session.change_shading = True
    state.update(change_shading=True)
    check()
    # save: the manager with the edited centres; reloaded, dest_color returns them
    saved = tmp_path / "edited"
    session.save(str(saved))
    back = ic.Cluster_Manager(cluster_config_file=str(saved), device=dev)
    assert back.class_num == 5 and back.clusters[3] is None
    px = torch.from_numpy(a32[0]).to(dev)
    got = back.dest_color(px, torch.from_numpy(flat_lab[0].reshape(-1, 1)).to(dev)).cpu()
    want_c, _ = E.update_img(a32[0], s32[0], r32[0], flat_lab[0], cls[0], centres)
    assert torch.equal(got, want_c) and not torch.equal(got, torch.from_numpy(a32[0]))
    assert torch.equal(mgr.clusters[0]["rgb_centers"].cpu(), _centres(lookup_tables["multi"])[0])        # the session's manager is untouched
    # the sine transfer through the session: the search and the cached form agree (its accuracy is test_sine_mode_against_fp64's)
    session.change_residual = True
    fresh = editing.EditSession(mgr, dev)
    fresh.add_frames_u8(albedo, shading, residual, lab)
    fresh.edit_centers.copy_(session.edit_centers)
    fresh.shading_scale, fresh.residual_scale, fresh.change_shading, fresh.change_residual = gs, gr, True, True
    maps = {"albedo_fine": torch.from_numpy(a32[1]).to(dev), "shading_fine": torch.from_numpy(s32[1]).to(dev),
            "residual_fine": torch.from_numpy(r32[1]).to(dev), "sem_label": torch.from_numpy(flat_lab[1].astype(np.float32)).to(dev)}
    assert np.array_equal(fresh.edit_render(maps, shape=(H, W)), session.frame(1))
    # reset: the originals
    session.reset()
    centres = _centres(session.tables)
    state = dict(change_shading=False, change_residual=False, shading_scale=1.0, residual_scale=1.0)
    assert not session.change_shading and not session.change_residual and session.shading_scale == 1.0 and session.residual_scale == 1.0
    assert torch.equal(session.edit_centers, session.centers)
    check()
    for i in range(F):
        assert np.array_equal(session.frame(i), snap_edit(i)[1])


@pytest.mark.parametrize("shaped", ["ssr", "object"])
def test_edit_render_equals_frame_on_the_same_pack(lookup_tables, shaped):
    """The novel-view edit (search form) and the resident frame (slots cached on first use, cached form afterwards) of one pack."""
    from intrinsicnerf_amd import editing, frames
    dev = _dev()
    H, W = 12, 16
    n = H * W
    ssr = shaped == "ssr"
    mgr = Manager(lookup_tables["clusters"] if ssr else [lookup_tables["clusters"][4]])
    pack_np, lab = E.edit_inputs(n, "random" if ssr else "ignore", mgr.class_num)
    g = torch.Generator().manual_seed(3)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    filler = lambda w: torch.rand(n, w, generator=g).to(dev)
    if ssr:
        maps = {"rgb_fine": filler(3), "disp_fine": filler(1), "depth_fine": filler(1), "albedo_fine": t(pack_np[:, 1:4]),
                "shading_fine": t(pack_np[:, 0]), "residual_fine": t(pack_np[:, 5:8]), "sem_label": t(pack_np[:, 4]), "sem_entropy": filler(1)}
    else:
        maps = {"rgb_map": filler(3), "disp_map": filler(1), "acc_map": filler(1), "albedo_map": t(pack_np[:, 1:4]),
                "shading_map": t(pack_np[:, 0]), "residual_map": t(pack_np[:, 5:8])}
    keys = list(maps)
    pack, widths = frames.pack_maps({k: v.reshape(n, -1) for k, v in maps.items()}, keys)
    session = editing.EditSession(mgr, dev)
    i = session.add_pack(pack, widths, keys, shape=(H, W))
    sem, k = (4, 4) if ssr else (0, 4)
    session.set_color(sem, k, 10, 200, 30)
    session.shading_scale, session.residual_scale, session.change_shading = 0.37, 1.63, True
    novel = session.edit_render(maps, shape=(H, W), c_albedo=True)
    first = session.frame(i, c_albedo=True)                            # search form, slots kept
    assert session._frames[i][0].slot is not None
    again = session.frame(i, c_albedo=True)                            # cached form
    for a, b, c in zip(novel, first, again):
        assert a.shape == (H, W, 3) and np.array_equal(a, b) and np.array_equal(a, c)
    assert np.array_equal(session.edit_render(maps), again[1].reshape(n, 3))
    # ... and it is the reference's line
    cls = _class_map(session.tables, t(pack_np), lab, not ssr)
    centres = _centres(session.tables)
    centres[sem][k] = torch.tensor([10 / 255.0, 200 / 255.0, 30 / 255.0])
    c_want, img = E.update_img(pack_np[:, 1:4], pack_np[:, 0], pack_np[:, 5:8], lab, cls, centres, change_shading=True, shading_scale=0.37,
                               residual_scale=1.63)
    assert np.array_equal(again[0].reshape(n, 3), E.to8b(c_want.numpy())) and np.array_equal(again[1].reshape(n, 3), E.to8b(img.numpy()))


def test_from_refresh_takes_the_kept_packs(lookup_tables):
    from intrinsicnerf_amd import editing, refresh
    dev = _dev()
    H, W = 3, 5
    n = H * W
    mgr = Manager(lookup_tables["clusters"])
    r = refresh.ClusterRefresh()
    r.device, r.H, r.W, r.n_frames, r.n_classes, r.manager = dev, H, W, 2, mgr.class_num, mgr
    with pytest.raises(RuntimeError):
        editing.EditSession.from_refresh(r)
    r.tables = lookup_tables["multi"]
    packs = []
    for f in range(2):
        pack_np, _ = E.edit_inputs(n, "random", mgr.class_num)
        pack_np[:, 1:4] = np.roll(pack_np[:, 1:4], f, 0)
        packs.append(pack_np)
        r._kept[f], r._cols[f] = torch.from_numpy(pack_np).to(dev), dict(E.COLS)
    session = editing.EditSession.from_refresh(r)
    assert session.n_frames == 2
    frames_ = [session.frame(f, c_albedo=True) for f in range(2)]
    for f in range(2):
        c, edit = r.snap(f)
        assert np.array_equal(frames_[f][0], c) and np.array_equal(frames_[f][1], edit)
