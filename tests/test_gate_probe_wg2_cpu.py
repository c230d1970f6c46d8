"""CPU: the resources of ``k_mlp_gate_probe_wg2_f16`` (csrc/mlp_f16_probe.h), the density gate's probe as two workgroups per CU.

Two four-wave workgroups share a CU only if each wave stays within 256 registers (two waves per SIMD) and two launches' LDS fit
the CU's 163 840 B; scratch would put a 128-accumulator wave tile's spills into the L2 the weight stream lives in.  The figures
come from the compiler's own report for gfx950 (``-Rpass-analysis=kernel-resource-usage``) on the library's flags."""
import os
import re
import shutil
import subprocess

import pytest

from intrinsicnerf_amd import _build

KERNEL = "k_mlp_gate_probe_wg2_f16"
CU_LDS_BYTES = 160 * 1024


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("probe_wg2") / "t128.o"
    flags = [f for f in _build.FLAGS if f != "-shared"]
    proc = subprocess.run([hipcc] + flags + ["-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(_build.CSRC, "mlp_f16_t128.hip"), "-o", str(out)],
                          capture_output=True, text=True)
    assert proc.returncode == 0, proc.stderr[-4000:]
    fields, name = {}, None
    for line in proc.stderr.split("\n"):
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if m and name:
            fields.setdefault(name, {})[m.group(1).strip()] = int(m.group(2))
    mine = [k for k in fields if KERNEL in k]
    assert len(mine) == 1, sorted(fields)
    assert not any(s in mine[0] for s in ("k_encode_mlp_f16x3_t128", "k_encode_mlp_f16x3_dual"))      # (tests/test_isa_audit_cpu.py counts by these)
    print(mine[0], fields[mine[0]])
    return fields[mine[0]]


def test_registers_and_scratch(usage):
    assert usage["ScratchSize"] == 0
    assert usage["VGPRs Spill"] == 0
    assert usage["VGPRs"] + usage["AGPRs"] <= 256
    assert usage["Occupancy"] >= 2


def test_two_launches_fit_the_cus_lds():
    """The launch size is a constant of the header (dynamic LDS: the compiler's report shows 0): the hi plane of 128 rows x 592 B and
    the parked encoding's extension, 128 rows x 3 pieces x 16 B - restated here, and tied to the header by its own static_assert
    (which the compile above has passed)."""
    src = open(os.path.join(_build.CSRC, "mlp_f16_probe.h")).read()
    assert re.search(r"kLdsBytesProbeWg2 = kPlaneT \* 2 \+ kProbeWg2ExtBytes;", src)
    assert re.search(r"kProbeWg2ExtBytes = kPtsT \* kParkExtPieces \* 16;", src)
    assert re.search(r"static_assert\(2 \* kLdsBytesProbeWg2 <= 160 \* 1024", src)
    launch = 128 * 592 + 128 * 3 * 16
    assert launch == 81920
    assert 2 * launch <= CU_LDS_BYTES
