"""The LDS-staged pair kernel's first feasible node, identity-like modes (NONE, DEFAULT).

A pod without a feasible match takes its first feasible node. NodeUnschedulable's verdict depends on
the pod only through its tolerates bit, so pair_lds_kernel computes that node once per wave and
tolerates value on the scalar unit (fn / ft during the scan, group_first_feasible_s after it) and a
lane selects one of the two. Every case forces the LDS form (pair_planes lds: small launches would
otherwise take the slice kernel) and compares idx / score / status bit-exact with the oracle.

The node tables place the first node feasible for a NON-tolerating pod at a chosen index (every node
below it is unschedulable) while the first node feasible for a tolerating pod stays node 0, so the two
answers differ: in group 0's lower or upper half, in the single lowest scan group, in the lower or
the upper group of a scan pair, only in the padded last group, or nowhere.
"""
from __future__ import annotations

import numpy as np
import pytest

from test_gpu_parity import _assert_same, _desc, _dev_batch, _plugins, _set

pytestmark = pytest.mark.gpu

LDS = {"pair_planes": "lds"}
NU, NN = ["NodeUnschedulable"], ["NodeNumber"]
IDENT = [(1, 0), (3, 0), (1, 1), (3, 1)]  # (weight, normalize): NONE and DEFAULT at weights 1 and 3
KXM = [(3, 2), (3, 3)]                    # REVERSE, MINMAX: unchanged code, one case per family
PODS = [1, 64, 65, 129, 512, 513]         # 129: a wave's second block is all padding lanes; 513: a second workgroup


def _table(n, first_nt, seed):
    """n nodes; every node below first_nt is unschedulable (None: every node), first_nt is not, the
    nodes above it are at random. Node digits 0-7 or none; digit 8 sits on exactly one node, which is
    unschedulable (only tolerating pods can match it), where the table has room for one; no node
    carries digit 9."""
    rng = np.random.default_rng(seed)
    u = (rng.random(n) < 0.3).astype(np.uint8)
    nd = rng.integers(0, 8, n).astype(np.int8)
    nd[rng.random(n) < 0.1] = -1
    if first_nt is None:
        u[:] = 1
    else:
        u[:first_nt] = 1
        u[first_nt] = 0
    k8 = 0 if u[0] else (n - 1 if n - 1 != first_nt else None)
    if k8 is not None:
        u[k8] = 1
        nd[k8] = 8
    return u, nd


def _pods(p, seed, flip=False):
    """Tolerating and non-tolerating pods mixed within the 64-lane blocks, the second block (pods
    64-127) tolerating only; digits 0-9 (8: the only matching node is unschedulable, 9: no node
    carries it) and pods without a digit."""
    rng = np.random.default_rng(seed)
    pd = rng.integers(0, 10, p).astype(np.int8)
    pd[rng.random(p) < 0.15] = -1
    pt = (rng.random(p) < 0.3).astype(np.uint8)
    pt[64:128] = 1
    if flip:
        pt ^= 1
    return pd, pt


def _check_modes(msh, oracle, ctx, u, nd, batches, modes, what):
    for w, norm in modes:
        ps = _plugins(oracle, NU, NN, NN, w, norm)
        _set(ctx, msh, ps)
        ctx.upload_nodes(u, nd)
        for pd, pt in batches:
            want = oracle.c_schedule_batch(u, nd, pd, pt, ps)
            _assert_same(ctx.schedule_batch(pd, pt), want, f"{what} w={w} norm={norm} p={len(pd)}")


# (nodes, index of the first node feasible for a non-tolerating pod or None, also REVERSE / MINMAX)
# Groups hold 256 nodes and tables are padded to 1,024 slots; the scan walks the groups above 0 in
# descending pairs and the lowest pair is the single group 1.
PLACES = [
    (1, 0, False), (1, None, False),                       # one node: group 0 holds padding
    (255, 0, False), (255, 128, False), (255, None, False),
    (256, 0, False), (256, 128, True), (256, None, False),  # group 0 full, groups 1-3 empty
    (257, 0, False), (257, 256, True), (257, None, False),  # node 256: alone in padded group 1 (the single lowest)
    (513, 256, False),                                     # group 1 full
    (513, 512, False),                                     # only the padded last group (lower of the pair 3, 2)
    (768, 256, False), (768, 512, False), (768, 767, False),  # group 3 empty, group 2 full: the pair's lower group
    (5000, 0, False), (5000, 200, False),                  # node 0; group 0's upper half
    (5000, 256, False),                                    # group 0 all unschedulable: the answers in different groups
    (5000, 2 * 256 + 7, True),                             # lower group of the pair (3, 2)
    (5000, 3 * 256 + 255, False),                          # upper group of the pair (3, 2)
    (5000, 18 * 256, False),                               # the highest full group, lower of the pair (19, 18)
    (5000, 19 * 256 + 135, True),                          # only the padded last group, its last real node
    (5000, None, True),                                    # nowhere
]


@pytest.mark.parametrize("n,first_nt,kx", PLACES)
def test_first_feasible_places(msh, oracle, n, first_nt, kx):
    """Each place of the first non-tolerating-feasible node x every pod count, NONE and DEFAULT at
    weights 1 and 3 (and REVERSE / MINMAX for one table per family). With every node unschedulable the
    non-tolerating pods end FitError and the tolerating ones still place."""
    u, nd = _table(n, first_nt, 7 * n + (first_nt or 0))
    batches = [_pods(p, 31 * n + p) for p in PODS] + [_pods(1, n, flip=True)]
    with msh.DeviceContext(0, LDS) as ctx:
        _check_modes(msh, oracle, ctx, u, nd, batches, IDENT + (KXM if kx else []), f"n={n} first_nt={first_nt}")
        if first_nt is None:  # the statuses the case is about, stated outright
            pd, pt = batches[-2]
            ps = _plugins(oracle, NU, NN, NN, 1, 0)
            _set(ctx, msh, ps)
            ctx.upload_nodes(u, nd)
            gi, _, gst = ctx.schedule_batch(pd, pt)
            assert (gst[pt == 0] == 1).all() and (gi[pt == 0] == -1).all()
            assert (gst[(pt == 1) & (pd >= 0)] == 0).all()


def test_only_match_unschedulable(msh, oracle):
    """Pods whose only matching node is unschedulable: a non-tolerating one falls to its first
    feasible node with score 0, a tolerating one takes the match."""
    n, first_nt = 5000, 700
    u, nd = _table(n, first_nt, 5)
    assert u[0] == 1 and nd[0] == 8 and (nd[1:] != 8).all()
    pd = np.full(200, 8, np.int8)
    pt = (np.arange(200) % 3 == 0).astype(np.uint8)
    with msh.DeviceContext(0, LDS) as ctx:
        _check_modes(msh, oracle, ctx, u, nd, [(pd, pt)], IDENT, "digit 8")
        gi, gs, gst = ctx.schedule_batch(pd, pt)  # the last mode set: DEFAULT, weight 3
        assert (gst == 0).all()
        assert (gi[pt == 1] == 0).all() and (gs[pt == 1] == 300).all()
        assert (gi[pt == 0] == first_nt).all() and (gs[pt == 0] == 0).all()


@pytest.mark.parametrize("w,norm", IDENT + KXM[1:])
def test_ragged_batches_launch(msh, oracle, w, norm):
    """One schedule_batches_device launch of ragged batches, a 0-pod and a 1-pod batch among them, on a
    table whose first non-tolerating-feasible node lies in the upper group of a scan pair."""
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda:0")
    n = 5000
    u, nd = _table(n, 5 * 256 + 3, 11)
    sizes = [513, 0, 1, 64, 65, 129, 1, 512, 1030]
    pods = [_pods(p, 100 + k, flip=(k == 6)) for k, p in enumerate(sizes)]
    ps = _plugins(oracle, NU, NN, NN, w, norm)
    with msh.DeviceContext(0, LDS) as ctx:
        _set(ctx, msh, ps)
        ctx.upload_nodes(u, nd)
        bufs = [_dev_batch(torch, dev, pd, pt, scores=(k % 4 != 3)) for k, (pd, pt) in enumerate(pods)]
        ctx.schedule_batches_device(ctx.batch_descs([_desc(t) for t in bufs]),
                                    stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        for k, (t, (pd, pt)) in enumerate(zip(bufs, pods)):
            want = oracle.c_schedule_batch(u, nd, pd, pt, ps)
            gi, gst = t[2].cpu().numpy(), t[4].cpu().numpy()
            gs = t[3].cpu().numpy() if t[3] is not None else want[1]
            _assert_same((gi, gs, gst), want, f"ragged batch {k} (p={len(pd)}) w={w} norm={norm}")


@pytest.mark.parametrize("w,norm", [(3, 1), (1, 0), (3, 3)])
def test_shard_keys_node_base(msh, oracle, w, norm):
    """shard_keys_device on two node shards, the second with a non-zero node_base: the second key of
    the identity-like modes is the same scalar first feasible node. The shards' keys merged by MAX and
    decoded equal the unsharded oracle. In shard 0 every node is unschedulable, so a non-tolerating
    pod's first feasible node comes from shard 1 (in its group 1) and a tolerating pod's from shard 0."""
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda:0")
    n, cut = 2000, 700
    u, nd = _table(n, cut + 300, 13)
    pd, pt = _pods(513, 17)
    ps = _plugins(oracle, NU, NN, NN, w, norm)
    want = oracle.c_schedule_batch(u, nd, pd, pt, ps)
    d_pd, d_pt = torch.from_numpy(pd).to(dev), torch.from_numpy(pt).to(dev)
    p = len(pd)
    st = torch.cuda.current_stream().cuda_stream
    merged, ctxs = None, []
    try:
        for a, b in ((0, cut), (cut, n)):
            c = msh.DeviceContext(0, LDS)
            ctxs.append(c)
            _set(c, msh, ps)
            c.upload_nodes(u[a:b], nd[a:b])
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


@pytest.mark.parametrize("first_nt", [0, 100 * 256 + 9, 128 * 256 + 231, None])
def test_sixteen_wave_form(msh, oracle, first_nt):
    """33,000 nodes (129 groups: 16-wave workgroups, the last group padded) x 2,048 pods: the first
    non-tolerating-feasible node at node 0, deep in the table, only in the padded last group, nowhere."""
    n = 33_000
    u, nd = _table(n, first_nt, 19)
    with msh.DeviceContext(0, LDS) as ctx:
        _check_modes(msh, oracle, ctx, u, nd, [_pods(2048, 23)], [(3, 1), (1, 0), (3, 3)], f"16-wave first_nt={first_nt}")
