"""The beam kernels' range checks in the debug build (``build/debug/_C.so``, -DMG_DEBUG, under
``MINGPT_DEBUG_CHECKS=1``; tests/test_debug_checks_gpu.py): a chosen candidate token outside the
vocabulary (merge) and a parent outside [0, W) (reorder) are clamped -- as in the release build, no
out-of-bounds access -- and reported by name.  Runs in a child process: one process holds one build
of the extension."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

CHILD = r'''
import torch
from mingpt_distributed_amd.ops._ext import DeviceCheckError, ext

C = ext()
assert C.debug_build(), "expected the MG_DEBUG build"
W, V, R, LH = 2, 100, 2, 4
i32 = lambda x: torch.tensor(x, dtype=torch.int32).cuda()
kv = torch.randn(1, R, 8, 3 * 16).to(torch.bfloat16).cuda()
keep = kv.clone()
C.beam_reorder(kv, W, i32([1, 0]), i32([8]))  # valid parents: no check fires
assert torch.equal(kv[0, 0, :, 16:], keep[0, 1, :, 16:]) and torch.equal(kv[0, 1, :, 16:], keep[0, 0, :, 16:])
try:
    C.beam_reorder(kv, W, i32([1, 7]), i32([8]))
except DeviceCheckError as e:
    assert "beam_reorder" in str(e), str(e)
    print("caught:", e)
else:
    raise AssertionError("beam_reorder: out-of-range parent not reported")
assert C.debug_error_bits() == 0
st = dict(score=torch.zeros(R).cuda(), fin=i32([0, 0]), len=i32([3, 3]), tok=torch.zeros(R, 1, dtype=torch.long).cuda(),
          parent=i32([0, 0]), hp=i32([[0] * LH] * R).view(1, W, LH), ht=i32([[0] * LH] * R).view(1, W, LH),
          hs=torch.zeros(1, W, LH).cuda(), pos=i32([2]), ctl=i32([1, -1, 9, 0]))
cand_tok, cand_c = i32([[V + 5, 1], [2, 3]]), torch.tensor([[-1.0, -2.0], [-3.0, -4.0]]).cuda()
try:
    C.beam_merge(W, V, cand_tok, cand_c, st["score"], st["fin"], st["len"], st["tok"], st["parent"], st["hp"],
                 st["ht"], st["hs"], st["pos"], st["ctl"])
except DeviceCheckError as e:
    assert "beam_merge" in str(e), str(e)
    print("caught:", e)
else:
    raise AssertionError("beam_merge: out-of-range token not reported")
assert st["tok"].view(-1).tolist() == [9, 1], st["tok"]  # clamped to the pad token
assert C.debug_error_bits() == 0
print("beam debug checks ok")
'''


def test_debug_build_reports_beam_indices():
    so = os.path.join(ROOT, "build", "debug", "_C.so")
    assert os.path.exists(so), "build/debug/_C.so missing: python build_ext.py --debug"
    env = dict(os.environ, MINGPT_EXT_SO=so, MINGPT_DEBUG_CHECKS="1", PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", CHILD], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=150)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "beam debug checks ok" in r.stdout
    assert r.stdout.count("caught:") == 2
