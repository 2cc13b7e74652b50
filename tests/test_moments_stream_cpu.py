"""Static checks of the compiled streaming moment kernel (k_moments_ring.hip; CPU-side: hipcc cross-compiles it to gfx950 assembly).
The kernel's header states its budget: at most 256 vector registers (two waves per SIMD), no scratch, 81 920 B of dynamic LDS per
workgroup (two workgroups in a CU's 160 KB); its LDS-DMA requests must take their LDS base from a wave-uniform value."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "gpz_amd", "csrc", "k_moments_ring.hip")
pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None, reason="needs hipcc")


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    asm = tmp_path_factory.mktemp("ring") / "k_moments_ring.s"
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                        "-I" + os.path.join(ROOT, "gpz_amd", "csrc"), "-S", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                        SRC, "-o", str(asm)], check=True, capture_output=True, text=True, timeout=900)
    return asm.read_text().splitlines(), r.stderr


def test_no_scratch_traffic_in_the_streaming_blocks(compiled):
    """No basic block of k_moments_ring that requests rows (global_load_lds), multiplies (v_mfma) or accumulates (v_fma_f64) touches
    scratch: a spill inside the loop is invisible to the parity tests and halves the rate."""
    lines, _ = compiled
    kernel = block = None
    nwork = nscratch = 0
    bad, seen = [], set()

    def close():
        if kernel and nwork and nscratch:
            bad.append((kernel, block, nwork, nscratch))

    for l in lines:
        m = re.match(r"^(_Z\w*k_moments_ring\w*):", l)
        if m:
            close()
            kernel, block, nwork, nscratch = m.group(1), "entry", 0, 0
            seen.add(kernel)
            continue
        if kernel is None:
            continue
        if l.startswith(".Lfunc_end"):
            close()
            kernel = None
            continue
        m = re.match(r"^(\.LBB\d+_\d+):", l)
        if m:
            close()
            block, nwork, nscratch = m.group(1), 0, 0
            continue
        t = l.strip()
        if t.startswith(("global_load_lds", "v_mfma", "v_fma_f64")):
            nwork += 1
        elif t.startswith("scratch_"):
            nscratch += 1
    assert len(seen) == 2, sorted(seen)            # d = 8 and d = 10
    assert not bad, bad


def test_lds_dma_base_is_never_picked_from_a_lane(compiled):
    """As tests/test_isa_guard.py for k_small / k_syrk_small: M0 (the LDS base of a request) must not be fed by a v_readfirstlane of a
    per-lane select, the mark of a request the compiler found under divergent control flow."""
    lines = [l.strip() for l in compiled[0]]
    assert any(l.startswith("global_load_lds_dwordx4") for l in lines)
    bad = []
    for i, l in enumerate(lines):
        m = re.match(r"s_mov_b32 m0, (s\d+)", l)
        if m and any(re.match(r"v_readfirstlane_b32 %s," % m.group(1), p) for p in lines[max(0, i - 8):i]):
            bad.append((i, lines[max(0, i - 3):i + 2]))
    assert not bad, bad[:3]


def test_registers_and_lds_are_inside_the_stated_budget(compiled):
    _, err = compiled
    src = open(SRC).read()
    dynamic = int(re.search(r"#define RG_LDS_BYTES (\d+)", src).group(1))
    slot = int(re.search(r"#define RG_SLOT_DOUBLES (\d+)", src).group(1))
    slots = int(re.search(r"#define RG_SLOTS (\d+)", src).group(1))
    cols = int(re.search(r"#define RG_COLS (\d+)", src).group(1))
    assert dynamic == 4 * slots * slot * 8 == 81920
    recs, cur = {}, None
    for l in err.splitlines():
        m = re.search(r"Function Name: (\S+)", l)
        if m:
            cur = m.group(1)
            recs[cur] = {}
            continue
        m = re.search(r"(VGPRs|AGPRs|ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]): (\d+)", l)
        if m and cur:
            recs[cur][m.group(1)] = int(m.group(2))
    ks = {k: v for k, v in recs.items() if "k_moments_ring" in k}
    assert len(ks) == 2, sorted(recs)
    for name, r in ks.items():
        assert r["VGPRs"] + r.get("AGPRs", 0) <= 256, (name, r)                            # two waves per SIMD
        assert r["ScratchSize [bytes/lane]"] == 0, (name, r)
        assert 2 * (r["LDS Size [bytes/block]"] + dynamic) <= 160 * 1024, (name, r)         # two workgroups per CU
    # PHI / T requested and not yet consumed in steady state: every slot but the one being read, 8 rows x cols x 16 B, 8 waves per CU
    assert 8 * (slots - 1) * 8 * cols * 16 >= 64 * 1024
