"""Static check of the chained hd = 64 attention backward (attn_bwdchain_kernel; no GPU needed): it
shares attn_bwd64_kernel's body with its inline-asm MFMAs, so the same operand hazards must be
absent (scripts/mfma_hazards.py --operands), and its private segment (scratch: a spill reload in
the tile loop waits for every load and store in flight) must not exceed the key-block kernel's."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_attention_bwdchain_hazards_and_scratch(tmp_path):
    out = tmp_path / "attn.s"
    c = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=fast", "-fno-slp-vectorize",
                        "--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage",
                        "-I" + os.path.join(ROOT, "csrc", "include"),
                        os.path.join(ROOT, "csrc", "kernels", "attention_train.hip"), "-o", str(out)],
                       check=True, capture_output=True, text=True)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "mfma_hazards.py"), str(out), "attn_bwdchain",
                        "--operands"], check=True, capture_output=True, text=True)
    lines = [l for l in r.stdout.splitlines() if "asm-MFMA operands" in l]
    assert len(lines) == 1 and lines[0].rstrip().endswith(": 0 asm-MFMA operands written < 2 wait states before or results read < 12 after"), r.stdout
    # the remarks list each kernel's name, then its figures
    scratch = {}
    name = None
    for l in c.stderr.splitlines():
        if m := re.search(r"Function Name: (\S+)", l):
            name = m.group(1)
        elif (m := re.search(r"ScratchSize \[bytes/lane\]: (\d+)", l)) and name:
            scratch[name] = int(m.group(1))
    chain = [v for k, v in scratch.items() if "attn_bwdchain_kernel" in k]
    keyblock = [v for k, v in scratch.items() if "attn_bwd64_kernel" in k]
    assert len(chain) == 1 and len(keyblock) == 1, sorted(scratch)
    assert chain[0] <= keyblock[0], (chain, keyblock)
