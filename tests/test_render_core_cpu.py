"""CPU: the chunk loop both front-ends share (render_core.render_chunks) and the draws wrapper next to it, driven by a stand-in
``piece`` that records ``(i, count, precision)`` and files f16 range words like a launch does - no device, no library."""
import warnings

import pytest
import torch


class _Piece:
    """Rays are their own index.  One range word per ``word_rays`` rays of a call (a single word for a call of no more than that),
    as the launches inside kernels.chunked_status keep them; ``trip``: the global ray indices at which a word starts that reports
    an out-of-range activation.  Values: the ray index in f16x3, 1000 + index in exact fp32."""

    def __init__(self, word_rays, trip=()):
        self.word_rays, self.trip, self.calls = word_rays, set(trip), []

    def __call__(self, i, count):
        from intrinsicnerf_amd import _capi, kernels
        prec = _capi.default_precision()
        self.calls.append((i, count, prec))
        if prec == _capi.PREC_F16X3:
            words = [_capi.STATUS_F16_RANGE if s in self.trip else 0 for s in range(i, i + count, self.word_rays)]
            kernels.check_f16_range(torch.tensor(words, dtype=torch.int32), "piece", deferrable=True)
        x = torch.arange(i, i + count, dtype=torch.float32) + (1000.0 if prec == _capi.PREC_F32 else 0.0)
        return {"x": x[:, None].repeat(1, 2), "y": x.clone()}


@pytest.fixture
def f16x3(monkeypatch):
    from intrinsicnerf_amd import _capi, kernels
    monkeypatch.setenv("INERF_PRECISION", "f16x3")
    assert _capi.default_precision() == _capi.PREC_F16X3
    yield _capi
    assert kernels._deferred is None and kernels._status_rays == 0


def _expected(n, f32_ranges):
    want = torch.arange(n, dtype=torch.float32)
    for a, b in f32_ranges:
        want[a:b] += 1000.0
    return want


def test_plain_loop_renders_only_the_tripped_chunk_again(f16x3):
    """(a) ``big == chunk``: 13 rays in chunks of 5, the middle one trips."""
    from intrinsicnerf_amd import render_core
    piece = _Piece(5, trip=[5])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out = render_core.render_chunks(piece, 13, 5, 5, "render")
    h, f = f16x3.PREC_F16X3, f16x3.PREC_F32
    assert piece.calls == [(0, 5, h), (5, 5, h), (10, 3, h), (5, 5, f)]
    assert torch.equal(out["y"], _expected(13, [(5, 10)]))
    assert torch.equal(out["x"], _expected(13, [(5, 10)])[:, None].repeat(1, 2))


def test_coalesced_loop_turns_both_tag_forms_into_spans(f16x3):
    """(b) 23 rays, ``chunk = 5``, ``big = 10``: word 1 of piece 0 (a tuple tag) and the single word of the 3-ray piece 2 (an int
    tag) trip; exactly (5, 5) and (20, 3) are rendered again, and the short tail is assigned in place."""
    from intrinsicnerf_amd import kernels, render_core
    seen_words = []

    class Piece(_Piece):
        def __call__(self, i, count):
            seen_words.append(kernels._status_rays)
            return super().__call__(i, count)

    piece = Piece(5, trip=[5, 20])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out = render_core.render_chunks(piece, 23, 5, 10, "render_rays")
    h, f = f16x3.PREC_F16X3, f16x3.PREC_F32
    assert piece.calls == [(0, 10, h), (10, 10, h), (20, 3, h), (5, 5, f), (20, 3, f)]
    assert seen_words == [5, 5, 5, 0, 0], "one range word per caller's chunk inside the loop only"
    assert torch.equal(out["y"], _expected(23, [(5, 10), (20, 23)]))
    assert out["x"].shape == (23, 2) and torch.equal(out["x"][:, 1], out["y"])


def test_fallback_warning_keeps_its_wording(f16x3, monkeypatch):
    from intrinsicnerf_amd import kernels, render_core
    monkeypatch.setattr(kernels, "_warned_fallback", False)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        render_core.render_chunks(_Piece(5, trip=[0, 10]), 13, 5, 5, "render")
    assert [str(w.message) for w in rec] == [
        "render: 2 of 3 chunks left the f16 range of the split-precision MLP kernel.  Re-running this batch with the exact fp32 "
        "MFMA kernel (set INERF_PRECISION=f32 to skip the attempt)."]


def test_no_rays_and_one_piece(f16x3):
    """(c) zero rays: ``{}`` without a call; (d) one piece: its own tensors, not a copy."""
    from intrinsicnerf_amd import render_core
    piece = _Piece(5)
    assert render_core.render_chunks(piece, 0, 5, 5, "render") == {} and piece.calls == []
    made = {}

    def one(i, count):
        made.update(_Piece(5)(i, count))
        return made

    out = render_core.render_chunks(one, 4, 5, 5, "render")
    assert set(out) == {"x", "y"} and all(out[k].data_ptr() == made[k].data_ptr() for k in out)
    out = render_core.render_chunks(one, 10, 5, 10, "render")          # (a coalesced frame of one piece)
    assert all(out[k].data_ptr() == made[k].data_ptr() for k in out)


class _Draws:
    steps = 0

    def advance(self):
        self.steps += 1


def test_draws_advance_once_after_the_last_chunk(f16x3, monkeypatch):
    """(e) the draws wrapper: one advance per loop, also when a piece raises; every piece of the object-level loop gets the global index
    of its first ray as ``ray_base``, the SSR loop's with ``with_ray_base``."""
    from intrinsicnerf_amd import object_level as ol, render_core, ssr
    draws = _Draws()
    out = render_core.advance_after(draws, render_core.render_chunks, _Piece(5), 13, 5, 5, "render")
    assert draws.steps == 1 and out["y"].shape == (13,)

    def broken(i, count):
        if i == 5:
            raise KeyError("piece")
        return _Piece(5)(i, count)

    with pytest.raises(KeyError):
        render_core.advance_after(draws, render_core.render_chunks, broken, 13, 5, 5, "render")
    assert draws.steps == 2
    bases = []
    monkeypatch.setattr(ol, "render_rays", lambda rb, draws=None, ray_base=None, **kw: (bases.append((rb.shape[0], ray_base)), {"y": rb[:, 0]})[1])
    rays = torch.arange(13, dtype=torch.float32)[:, None].expand(13, 11).contiguous()
    out = ol.batchify_rays(rays, 5, draws=draws, perturb=1.0, ray_base=100)
    assert bases == [(5, 100), (5, 105), (3, 110)] and draws.steps == 3 and torch.equal(out["y"], rays[:, 0])
    bases.clear()
    ol.batchify_rays(rays, 5, draws=draws, perturb=0., raw_noise_std=0.)       # nothing drawn: the step counts drawing renders
    assert bases == [(5, 0), (5, 5), (3, 10)] and draws.steps == 3
    bases.clear()
    ol.batchify_rays(rays, 5, perturb=1.0)                                     # torch's generator: no base
    assert bases == [(5, None), (5, None), (3, None)] and draws.steps == 3
    out = ssr.batchify_rays(lambda rb, ray_base=None: (bases.append(ray_base), {"y": rb[:, 0]})[1], rays, 5, with_ray_base=True)
    assert bases[3:] == [0, 5, 10] and torch.equal(out["y"], rays[:, 0])
