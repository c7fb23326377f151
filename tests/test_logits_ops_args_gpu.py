"""The argument checks that the five logits-row ops share (csrc/bindings.cpp: ``sample_logits``,
``sample_kept``, ``pick_ragged``, ``logits_lse``, ``beam_rows``): a logits tensor the row kernels
cannot read in 16-byte loads, a column count outside it, or a malformed parameter block is refused
on the host with a RuntimeError that names the op, and nothing is launched -- the buffers the op
would write keep their sentinels.

Not repeated here: what tests/test_sample_kernel_gpu.py::test_binding_rejects_bad_arguments already
asserts for ``sample_logits`` (V past the columns, fp32 logits, a short parameter block, a row stride
that is no multiple of 8).  fp32 logits are refused by the dtype check every binding shares, whose
message names the argument, not the op."""
import pytest
import torch

pytestmark = pytest.mark.gpu

B, N = 2, 16
SENTINEL = -7
OPS = ["sample_logits", "sample_kept", "pick_ragged", "logits_lse", "beam_rows"]
WITH_PARAMS = OPS[:3]


@pytest.fixture(scope="module")
def C():
    from mingpt_distributed_amd.ops._ext import ext

    return ext()


def bf16(rows, cols):
    return torch.zeros(rows, cols, dtype=torch.bfloat16, device="cuda")


# name -> (logits [2, <= 16], V): one thing wrong with each
LOGITS_CASES = {
    "column_stride_2": lambda: (bf16(B, 2 * N)[:, ::2], N),
    "V_0": lambda: (bf16(B, N), 0),
    "V_past_columns": lambda: (bf16(B, N), N + 1),
    "row_stride_20": lambda: (bf16(B, 20)[:, :N], N),
    "base_off_16_bytes": lambda: (bf16(B, N)[:, 1:], N - 1),
    "fp32": lambda: (bf16(B, N).float(), N),
}
PARAMS_CASES = {
    "params_7_words": lambda: torch.zeros(7, dtype=torch.int32, device="cuda"),
    "params_int64": lambda: torch.zeros(8, dtype=torch.long, device="cuda"),
}
COVERED = {("sample_logits", c) for c in ("V_past_columns", "fp32", "params_7_words", "row_stride_20")}
CASES = [(op, c) for op in OPS for c in LOGITS_CASES if (op, c) not in COVERED]
CASES += [(op, c) for op in WITH_PARAMS for c in PARAMS_CASES if (op, c) not in COVERED]


def call(C, op, logits, V, params, out):
    """Run ``op`` on (logits, V, params) with every other argument well-formed; ``out`` (a list)
    receives the caller-owned buffers the op would write, filled with SENTINEL, before the call."""
    rows = logits.size(0)
    i32 = lambda *s: torch.full(s, SENTINEL, dtype=torch.int32, device="cuda")
    f32 = lambda *s: torch.full(s, float(SENTINEL), dtype=torch.float32, device="cuda")
    i64 = lambda *s: torch.full(s, SENTINEL, dtype=torch.long, device="cuda")
    try:
        if op == "sample_logits":
            C.sample_logits(logits, V, params)
        elif op == "sample_kept":
            C.sample_kept(logits, V, params)
        elif op == "logits_lse":
            C.logits_lse(logits, V)
        elif op == "pick_ragged":
            pos, done = torch.zeros(rows, dtype=torch.int32, device="cuda"), torch.zeros(rows, dtype=torch.int32,
                                                                                         device="cuda")
            out += [i64(rows), i64(rows, 4)]
            C.pick_ragged(logits, V, params, pos, done, out[0], out[1], True)
        else:
            score, fin = torch.zeros(rows, device="cuda"), torch.zeros(rows, dtype=torch.int32, device="cuda")
            ctl = torch.zeros(4, dtype=torch.int32, device="cuda")
            out += [i32(rows, 1), f32(rows, 1), f32(rows, 2)]
            C.beam_rows(logits, V, 1, score, fin, ctl, *out)
    finally:
        torch.cuda.synchronize()


@pytest.mark.parametrize("op,case", CASES, ids=[f"{op}-{c}" for op, c in CASES])
def test_rejected_before_launch(C, op, case):
    params = torch.zeros(8, dtype=torch.int32, device="cuda")
    logits, V = bf16(B, N), N
    if case in LOGITS_CASES:
        logits, V = LOGITS_CASES[case]()
    else:
        params = PARAMS_CASES[case]()
    outs = []
    with pytest.raises(RuntimeError, match="bf16" if case == "fp32" else op):
        call(C, op, logits, V, params, outs)
    for o in outs:
        assert (o == SENTINEL).all(), "the op wrote before it refused"


def test_well_formed_call_passes(C):
    """The same helper with nothing wrong runs every op: the cases above fail for their one reason."""
    params = torch.zeros(8, dtype=torch.int32, device="cuda")
    params[3] = 0x3F800000  # inv_t = 1.0
    for op in OPS:
        call(C, op, bf16(B, N), N, params, [])
