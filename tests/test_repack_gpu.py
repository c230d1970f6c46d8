"""GPU: inerf_repack (the library's own device-side re-packing: a memset + three kernels that read the parameters where they
live) against the host packer (inerf_pack_weights / inerf_pack_weights_bwd) - bit for bit, both blobs, object-level and SSR
networks, including an all-zero GEMM, a rescaled one and a non-contiguous parameter.  (The framework-operation twin that the
CPU tests pin to the host packer is bit-identical on the CPU only: run on the GPU it differs from the host packer in about a
third of the halves - another valid hi/lo split, hi rounded differently and lo compensating; the first GPU run of this test
found that - so the training steps of rounds 1-2 used blobs that were not the host packer's; the library's kernels are now the
device path.)"""
import pytest
import torch

import oracle

pytestmark = pytest.mark.gpu


def _desc(variant, c, l_xyz=10, l_dir=4):
    from intrinsicnerf_amd import _capi
    return _capi.net_desc(_capi.VARIANT_SSR if variant == "ssr" else _capi.VARIANT_OBJECT, c, l_xyz, l_dir, 10.0 if variant == "ssr" else 1.0,
                          precision=_capi.PREC_F16X3)


CASES = [("object", 0, 10, 4), ("ssr", 28, 10, 4), ("ssr", 101, 10, 4), ("ssr", 0, 10, 4),
         # reduced encodings (where the pad columns start) and the class edges 129 / 240
         ("object", 0, 6, 2), ("object", 0, 0, 0), ("ssr", 240, 6, 2), ("ssr", 129, 10, 4)]


@pytest.mark.parametrize("variant,c,l_xyz,l_dir", CASES,
                         ids=[f"{v}-{c}" if (lx, ld) == (10, 4) else f"{v}-{c}-x{lx}d{ld}" for v, c, lx, ld in CASES])
def test_hip_repack_is_bit_identical_to_the_host_packer(variant, c, l_xyz, l_dir, monkeypatch):
    from intrinsicnerf_amd import packing
    dev = torch.device("cuda:0")
    desc = _desc(variant, c, l_xyz, l_dir)
    for seed in (3, 4):
        sd = oracle.make_state_dict(variant, c, seed=seed, l_xyz=l_xyz, l_dir=l_dir)
        if seed == 4:
            sd["pts_linears.2.weight"] = sd["pts_linears.2.weight"] * 0.0          # an all-zero GEMM: scale 1
            sd["feature_linear.weight"] = sd["feature_linear.weight"] * 1000.0     # moves the common scale of the d h7 group
            sd["views_linears.0.weight"] = sd["views_linears.0.weight"].t().contiguous().t()      # a non-contiguous parameter
        sd_dev = {k: v.to(dev) for k, v in sd.items()}
        for backward in (False, True):
            host = packing.pack_state_dict_bwd(desc, sd) if backward else packing.pack_state_dict(desc, sd)
            packer = packing.DevicePacker(desc, backward, dev)
            assert packer.hip is not None
            got = packer(sd_dev)                       # the library's inerf_repack
            twin = packer._repack_torch(sd_dev)        # its framework twin (what CPU tensors take)
            torch.cuda.synchronize()
            assert torch.equal(host.view(torch.int32), got.cpu().view(torch.int32)), (variant, c, l_xyz, l_dir, seed, backward, "hip vs host")
            differing = int((twin.view(torch.int16) != got.view(torch.int16)).sum())
            print(f"{variant} C={c} ({l_xyz}, {l_dir}) seed {seed} {'bwd' if backward else 'fwd'}: framework twin differs from the host packer in {differing} of "
                  f"{2 * got.numel()} halves")
