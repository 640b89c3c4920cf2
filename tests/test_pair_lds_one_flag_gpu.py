"""pair_lds_kernel, identity-like modes (NONE, DEFAULT): one match flag per lane for the whole scan,
the upward walk of a lane whose first match lies above group 0, and group 0's first match from dm'
alone (no V plane). Every case forces the LDS form (pair_planes lds) and compares idx / score / status
bit-exact with the oracle in NONE and DEFAULT at weights 1 and 3.

The tables come from pair_one_flag_cases; before each GPU call the case asserts, from the oracle's
expected indices, that its targeted pods resolve above group 0 on the intended node and the others
inside it (tests/test_pair_lds_one_flag.py checks the same without a GPU).
"""
from __future__ import annotations

import numpy as np
import pytest

import pair_one_flag_cases as C
from test_gpu_parity import _assert_same, _desc, _dev_batch, _plugins, _set

pytestmark = pytest.mark.gpu

LDS = {"pair_planes": "lds"}
NU, NN = ["NodeUnschedulable"], ["NodeNumber"]


@pytest.fixture(scope="module")
def lds_ctx(msh):
    with msh.DeviceContext(0, LDS) as ctx:
        yield ctx


def _run_case(msh, oracle, ctx, case, counts):
    batches = [C.pods(p) for p in counts]
    for w, norm in reversed(C.IDENT):  # DEFAULT, weight 3 first: the mode the coverage proof reads
        ps = _plugins(oracle, NU, NN, NN, w, norm)
        _set(ctx, msh, ps)
        ctx.upload_nodes(case.u, case.nd)
        for pd, pt in batches:
            want = oracle.c_schedule_batch(case.u, case.nd, pd, pt, ps)
            if (w, norm) == (3, 1):
                C.check_coverage(case, pd, pt, want[0], want[2])
            _assert_same(ctx.schedule_batch(pd, pt), want, f"{case.name} w={w} norm={norm} p={len(pd)}")


@pytest.mark.parametrize("case", C.above_cases(), ids=lambda c: c.name)
def test_first_match_above_group0(msh, oracle, lds_ctx, case):
    """The first match in group 1, a middle group, the last full group or the padded last group, as a
    word's first or last node; non-tolerating and tolerating pods of one digit get different answers;
    each 64-pod block mixes lanes resolved in group 0, above it in different groups and nowhere, pods
    without a digit and padding lanes; 1 to 513 pods."""
    _run_case(msh, oracle, lds_ctx, case, C.PODS)


@pytest.mark.parametrize("case", C.group0_cases(), ids=lambda c: c.name)
def test_group0_first_match(msh, oracle, lds_ctx, case):
    """Group 0's first match at node 0, 31, 32, 127, 128 and 255, in tables below 256 nodes (group 0
    holds padding, which no V plane masks any more), and with the digit's only node unschedulable."""
    _run_case(msh, oracle, lds_ctx, case, C.PODS)


def test_ragged_batches_one_launch(msh, oracle, lds_ctx):
    """Three batches of 130, 0 and 65 pods in one launch on the 5-group table."""
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda:0")
    case = C.above_case(1100, 3 * C.G + 255, 2 * C.G + 96, 4 * C.G + 1)
    batches = [C.pods(130), C.pods(0), C.pods(65, shift=7)]
    for w, norm in C.IDENT:
        ps = _plugins(oracle, NU, NN, NN, w, norm)
        _set(lds_ctx, msh, ps)
        lds_ctx.upload_nodes(case.u, case.nd)
        wants = [oracle.c_schedule_batch(case.u, case.nd, pd, pt, ps) for pd, pt in batches]
        if (w, norm) == (3, 1):
            for (pd, pt), want in zip(batches, wants):
                if len(pd):
                    C.check_coverage(case, pd, pt, want[0], want[2])
        bufs = [_dev_batch(torch, dev, pd, pt) for pd, pt in batches]
        lds_ctx.schedule_batches_device(lds_ctx.batch_descs([_desc(t) for t in bufs]),
                                        stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        for k, (t, want) in enumerate(zip(bufs, wants)):
            _assert_same([t[i].cpu().numpy() for i in (2, 3, 4)], want, f"ragged batch {k} w={w} norm={norm}")


@pytest.mark.parametrize("w,norm", [(3, 1), (1, 0)])
def test_shard_keys_node_base(msh, oracle, w, norm):
    """shard_keys_device on two node shards: in the second (node_base 700) the targeted lanes find their
    first match above that shard's own group 0. The keys merged by MAX and decoded equal the oracle on
    the whole table."""
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda:0")
    case, cut = C.shard_case()
    n = len(case.u)
    pd, pt = C.pods(513)
    ps = _plugins(oracle, NU, NN, NN, w, norm)
    want = oracle.c_schedule_batch(case.u, case.nd, pd, pt, ps)
    if (w, norm) == (3, 1):
        assert C.check_coverage(case, pd, pt, want[0], want[2], base=cut) > 0
    d_pd, d_pt = torch.from_numpy(pd).to(dev), torch.from_numpy(pt).to(dev)
    p = len(pd)
    st = torch.cuda.current_stream().cuda_stream
    merged, ctxs = None, []
    try:
        for a, b in ((0, cut), (cut, n)):
            c = msh.DeviceContext(0, LDS)
            ctxs.append(c)
            _set(c, msh, ps)
            c.upload_nodes(case.u[a:b], case.nd[a:b])
            keys = torch.full((c.shard_keys_len(p),), -7, dtype=torch.int32, device=dev)
            c.shard_keys_device(p, d_pd.data_ptr(), d_pt.data_ptr(), a, keys.data_ptr(), st)
            assert int(keys.min()) >= 0  # every entry written
            merged = keys if merged is None else torch.maximum(merged, keys)
        out = _dev_batch(torch, dev, pd, pt)
        ctxs[0].decode_keys_device(p, d_pd.data_ptr(), d_pt.data_ptr(), merged.data_ptr(), out[2].data_ptr(),
                                   out[3].data_ptr(), out[4].data_ptr(), st)
        torch.cuda.synchronize()
        _assert_same([out[i].cpu().numpy() for i in (2, 3, 4)], want, f"shard keys w={w} norm={norm}")
    finally:
        for c in ctxs:
            c.close()


def test_sixteen_wave_instance(msh, oracle, lds_ctx):
    """129 groups (33,024 nodes, the 16-wave workgroups) x 300 pods: digit 7's first match is the
    table's last node, digit 8's in groups 64 and 100."""
    _run_case(msh, oracle, lds_ctx, C.big_case(), [300])
