"""GPU: the density gate's raw rows where a sub-range of the launch does not start on a sixteen-byte boundary.

The trunk and probe kernels store a group's 16 rows x 11 floats as 44 sixteen-byte pieces and fall back to four-byte stores when the
sub-range's ``raw`` is not sixteen-byte aligned (``store_sigma_rows``, csrc/mlp_f16_gate.h).  A sub-range starts r0 * S * 44 bytes into
``raw``: with 193 samples and sub-ranges of 3 rays the offsets are 0, 25 476 and 50 952 bytes - 0, 4 and 8 modulo 16 - so the second and
third sub-range take the fallback in every group, and their 579 and 193 points are no multiple of 16 or 128 (ragged groups and tiles).

7 rays x 193 samples = 1 351 points of the bench sample through the fine network; fp64 model of this input (tests/_gate_probe.py): live /
candidate / all points per sub-range 202 / 306 / 579, 132 / 207 / 579, 50 / 69 / 193; smallest |sigma| 1.1e-4, three orders above the f16x3
error - no point's sign is in doubt."""
import pytest
import torch

import _gate_probe as gp

pytestmark = pytest.mark.gpu

N_RAYS, N_SAMPLES, RAYS_PER_SUB = 7, 193, 3


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    for k in ("INERF_PRECISION", "INERF_F16_KERNEL", "INERF_GATE", "INERF_PROBE", "INERF_PROBE_WG", "INERF_GATE_LOG", "INERF_ENC_CACHE",
              "INERF_GATE_BYTES"):
        monkeypatch.delenv(k, raising=False)


def _bits(t):
    return t.contiguous().view(torch.int32)


def test_rows_of_sub_ranges_off_the_sixteen_byte_boundary(monkeypatch):
    from intrinsicnerf_amd import _capi, kernels, packing
    assert (RAYS_PER_SUB * N_SAMPLES * 11) % 4 != 0          # the premise: the second sub-range's rows start off a sixteen-byte boundary
    dev = torch.device("cuda:0")
    sd, rays = gp.network("bench_fine")
    desc = _capi.net_desc(_capi.VARIANT_OBJECT, precision=_capi.PREC_F16X3)
    packed = packing.pack_state_dict(desc, sd).to(dev)
    rays = rays[::585][:N_RAYS].contiguous()
    assert rays.shape[0] == N_RAYS
    z = gp.sample_depths(rays, N_SAMPLES, seed=23).to(dev)
    rays = rays.to(dev)
    n = N_RAYS * N_SAMPLES
    monkeypatch.setenv("INERF_GATE_BYTES", str(RAYS_PER_SUB * N_SAMPLES * 1028))      # sub-ranges of 3, 3 and 1 rays

    def run(**kw):
        raw = kernels.encode_mlp(desc, packed, rays, z, **kw)
        torch.cuda.synchronize()
        assert raw.data_ptr() % 16 == 0                      # (the first sub-range is aligned: the offsets above are the whole story)
        return raw.reshape(n, 11)

    def probed():
        po = torch.full((n, 2), float("nan"), device=dev)
        return run(gate_colour=True, gate_probe=True, probe_out=po), po

    plain = run()
    raw_wg2, po_wg2 = probed()
    monkeypatch.setenv("INERF_PROBE_WG", "1")
    raw_wg1, po_wg1 = probed()
    monkeypatch.delenv("INERF_PROBE_WG")
    raw_trunk = run(gate_colour=True, gate_probe=False)

    # the two probe forms: the same bits, every point written
    assert not bool(torch.isnan(po_wg2).any()) and not bool(torch.isnan(po_wg1).any())
    assert torch.equal(_bits(po_wg2), _bits(po_wg1))
    assert torch.equal(_bits(raw_wg2), _bits(raw_wg1))

    live = plain[:, 3] > 0
    first = [0, RAYS_PER_SUB * N_SAMPLES, 2 * RAYS_PER_SUB * N_SAMPLES, n]
    for a, b in zip(first[:-1], first[1:]):                  # every sub-range has points on both sides
        k = int(live[a:b].sum())
        print(f"points {a}..{b}: {k} live of {b - a}")
        assert 0 < k < b - a
    dead = ~live                                             # live | dead = every point: none is left out of the comparisons
    for name, raw in (("probe, two workgroups", raw_wg2), ("probe, eight waves", raw_wg1), ("no probe", raw_trunk)):
        assert torch.equal(_bits(raw[live]), _bits(plain[live])), name                        # all eleven channels
        colours = raw[dead][:, [0, 1, 2, 4, 5, 6, 7, 8, 9, 10]]
        assert bool((_bits(colours) == 0).all()), name                                         # +0.0
        assert bool((raw[dead][:, 3] <= 0).all()), name
    assert torch.equal(_bits(raw_trunk[:, 3]), _bits(plain[:, 3]))                             # the exact trunk's sigma at every point
