"""Build-time guard on the registers of the decode GEMVs (hipcc cross-compiles gemv.hip for gfx950 without a GPU and reports every
kernel's resources: -Rpass-analysis=kernel-resource-usage).

The packed policy WP12 streams DEPTH chunks per row of 3 VGPRs each, and the depth only pays while the waves stay resident: the law of
profiles/r04_stream_layout_bench.txt is bytes in flight per CU = waves x bytes per wave.  So every WP12 instantiation must keep no
scratch and no VGPR spill, the row kernels 4 waves per SIMD (4 workgroups per CU: 16 waves x 9 KB = 144 KB in flight) and the K-split
kernel without the fused norm -- down_proj's -- 7 (its 7 workgroups per CU stay resident: 28 waves x 4.5 KB = 126 KB).  And the depth is
WP12's alone: every other kernel of the file has the VGPR count it had before (tests/golden/gemv_resources.json)."""
import json
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "streamvln_amd", "csrc", "gemv.hip")
GOLD = os.path.join(ROOT, "tests", "golden", "gemv_resources.json")
REMARK = re.compile(r"remark: (?:\S+:\d+:\d+: )?\s*(.*?): (.*?) \[-Rpass-analysis=kernel-resource-usage\]")


@pytest.fixture(scope="module")
def resources():
    """{kernel: {field: value}} of one device-only compile of gemv.hip"""
    if shutil.which("hipcc") is None:
        pytest.skip("needs hipcc")
    with tempfile.TemporaryDirectory() as d:
        r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                            "-c", "-o", os.path.join(d, "gemv.o"), SRC], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    out, cur = {}, None
    for ln in r.stderr.splitlines():
        m = REMARK.search(ln)
        if not m:
            continue
        key, val = m.group(1).strip(), m.group(2).strip()
        if key == "Function Name":
            cur = out.setdefault(val, {})
        elif cur is not None:
            cur[key] = val
    return out


def test_wp12_kernels_keep_their_waves_and_spill_nothing(resources):
    wp12 = {k: v for k, v in resources.items() if "WP12" in k}
    rows = [k for k in wp12 if "gemv_rows_kernel" in k]
    ksplit = [k for k in wp12 if "gemv_ksplit_kernel" in k]
    assert len(rows) >= 9 and len(ksplit) == 2 and len(rows) + len(ksplit) == len(wp12), sorted(wp12)
    for k, v in wp12.items():
        print(k, v["VGPRs"], v["Occupancy [waves/SIMD]"])
        assert int(v["ScratchSize [bytes/lane]"]) == 0 and int(v["VGPRs Spill"]) == 0, (k, v)
        assert v["Dynamic Stack"] == "False", (k, v)
    for k in rows:
        assert int(wp12[k]["Occupancy [waves/SIMD]"]) >= 4 and int(wp12[k]["VGPRs"]) <= 128, (k, wp12[k])
    for k in ksplit:
        assert int(wp12[k]["Occupancy [waves/SIMD]"]) >= 7 and int(wp12[k]["VGPRs"]) <= 72, (k, wp12[k])


def test_the_other_kernels_have_the_registers_they_had(resources):
    want = json.load(open(GOLD))["vgprs"]
    got = {k: int(v["VGPRs"]) for k, v in resources.items() if "WP12" not in k}
    assert set(got) == set(want), sorted(set(got) ^ set(want))[:6]
    diff = {k: (want[k], got[k]) for k in want if want[k] != got[k]}
    assert not diff, diff
