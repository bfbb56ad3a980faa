"""Batched segmentation calls (SegBatch: one launch per kernel for the blocks of a stage) against the per-handle entry points
on the same inputs.  Those are pinned by reference-made goldens (test_seg_gpu.py); everything here is integers, so equality is
exact.  Edge lists leave the hash table in any order: compared after sorting by (u, v)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

MSD, FILT, DEBRIS = 4, 0.35, 12
SMALL = dict(shape=(11, 40, 56), crop_offset=(1, 4, 4), n=5)        # 11 slices: the last flood workgroup (8 slices each) is partly filled
SLICE160 = dict(shape=(9, 160, 160), crop_offset=(1, 4, 4), n=3, plain=True)    # the bench's slice: the seed kernel's full LDS footprint
LABEL_CAP, EDGE_CAP = 4096, 1 << 15


def blobby(shape, seed):
    from scipy.ndimage import gaussian_filter
    rng = np.random.default_rng(seed)
    a = gaussian_filter(rng.random((3,) + tuple(shape)), sigma=(0, 1, 3, 3))
    return ((a - a.min()) / (a.max() - a.min()) * 255).astype(np.uint8)


def block_inputs(shape, n, plain=False):
    """n blocks: blobby ones with different seeds; unless `plain`, the last two are an all-zero and an all-255 one"""
    blocks = [blobby(shape, 100 + i) for i in range(n if plain else n - 2)]
    if not plain:
        blocks += [np.zeros((3,) + tuple(shape), np.uint8), np.full((3,) + tuple(shape), 255, np.uint8)]
    return [torch.from_numpy(b).cuda() for b in blocks]


@pytest.fixture(scope="module")
def engines():
    from bootstrapper_amd.post.engine import SegEngine
    return [SegEngine((11, 160, 160), 0) for _ in range(5)]


def crop_of(case):
    return tuple(s - 2 * c for s, c in zip(case["shape"], case["crop_offset"]))


def sorted_graph(edges, sums, cnts, counts):
    ne = int(counts[0])
    e, s, c = edges[:ne].cpu().numpy(), sums[:ne].cpu().numpy(), cnts[:ne].cpu().numpy()
    o = np.lexsort((e[:, 1], e[:, 0]))
    return e[o], s[o], c[o], counts[:3].cpu().numpy()


def single_block(eng, affs, case, id_offset, edge_cap=EDGE_CAP):
    """the per-handle calls of one block: fragments, clean-up + crop + relabel, node statistics; the region graph of the filtered fragments"""
    fr, mx = eng.ws_fragments(affs, True, MSD)
    lab, num = eng.postprocess_fragments(affs, fr, FILT, DEBRIS, case["crop_offset"], crop_of(case), id_offset)
    size = torch.empty(LABEL_CAP, dtype=torch.int64, device="cuda")
    sums = torch.empty((LABEL_CAP, 3), dtype=torch.int64, device="cuda")
    eng.label_stats(lab, id_offset, LABEL_CAP, size=size, sums=sums)
    g = graph_buffers(edge_cap)
    eng.rag_graph_async(affs, fr, *g)
    eng.status()
    return dict(frags=fr.cpu().numpy(), max_id=int(mx.item()), labels=lab.cpu().numpy(), num=int(num.item()), size=size.cpu().numpy(),
                sums=sums.cpu().numpy(), graph=sorted_graph(*g))


def graph_buffers(cap):
    return (torch.empty((cap, 2), dtype=torch.int64, device="cuda"), torch.empty(cap, dtype=torch.int64, device="cuda"),
            torch.empty(cap, dtype=torch.int32, device="cuda"), torch.zeros(4, dtype=torch.int64, device="cuda"))


_REF = {}


def reference(engines, name, case):
    """computed once per case, shared by the tests and left unchanged"""
    if name not in _REF:
        affs = block_inputs(case["shape"], case["n"], case.get("plain", False))
        _REF[name] = (affs, [single_block(engines[0], a, case, 1000 * (i + 1)) for i, a in enumerate(affs)])
    return _REF[name]


def batched_fragments(batch, affs, case, rows):
    n = len(rows)
    fr = [torch.empty(case["shape"], dtype=torch.int64, device="cuda") for _ in range(n)]
    lab = [torch.empty(crop_of(case), dtype=torch.int64, device="cuda") for _ in range(n)]
    nums = [torch.zeros(1, dtype=torch.int64, device="cuda") for _ in range(n)]
    size = [torch.empty(LABEL_CAP, dtype=torch.int64, device="cuda") for _ in range(n)]
    sums = [torch.empty((LABEL_CAP, 3), dtype=torch.int64, device="cuda") for _ in range(n)]
    mx = batch.fragments([affs[r] for r in rows], fr, lab, nums, [1000 * (r + 1) for r in rows], size, sums, MSD, FILT, DEBRIS, case["crop_offset"])
    for e in batch.engines[:n]:
        e.status()
    return fr, lab, nums, size, sums, mx


def check_fragments(ref, fr, lab, num, size, sums, mx):
    assert np.array_equal(fr.cpu().numpy(), ref["frags"])
    assert int(mx.item()) == ref["max_id"]
    assert int(num.item()) == ref["num"]
    assert np.array_equal(lab.cpu().numpy(), ref["labels"])
    assert np.array_equal(size.cpu().numpy(), ref["size"]) and np.array_equal(sums.cpu().numpy(), ref["sums"])


def check_graph(ref, got):
    for a, b in zip(ref["graph"], got):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("name,case", [("small", SMALL), ("slice160", SLICE160)])
def test_fragments_and_graph_equal_the_single_block_calls(engines, name, case):
    from bootstrapper_amd.post.engine import SegBatch
    affs, refs = reference(engines, name, case)
    n = case["n"]
    batch = SegBatch(engines[:n])   # (small: N = the number of workspaces)
    fr, lab, nums, size, sums, mx = batched_fragments(batch, affs, case, list(range(n)))
    assert all(r["num"] > 0 for r in refs[:n - 2])
    for i in range(n):
        check_fragments(refs[i], fr[i], lab[i], nums[i], size[i], sums[i], mx[i])
    bufs = [graph_buffers(EDGE_CAP) for _ in range(n)]
    batch.rag_graph(affs, fr, *[list(x) for x in zip(*bufs)])
    for e in engines[:n]:
        e.status()
    assert max(int(r["graph"][3][0]) for r in refs) > 10
    for i in range(n):
        check_graph(refs[i], sorted_graph(*bufs[i]))


def test_one_block_in_a_batch_of_five_workspaces(engines):
    from bootstrapper_amd.post.engine import SegBatch
    affs, refs = reference(engines, "small", SMALL)
    batch = SegBatch(engines)
    for r in (0, 2):   # two calls queued back to back on the same row of the table
        fr, lab, nums, size, sums, mx = batched_fragments(batch, affs, SMALL, [r])
        check_fragments(refs[r], fr[0], lab[0], nums[0], size[0], sums[0], mx[0])
        g = graph_buffers(EDGE_CAP)
        batch.rag_graph([affs[r]], fr, [g[0]], [g[1]], [g[2]], [g[3]])
        engines[0].status()
        check_graph(refs[r], sorted_graph(*g))


def test_an_overflow_marks_its_own_workspace_only(engines):
    from bootstrapper_amd import _lib
    from bootstrapper_amd.post.engine import SegBatch
    affs, refs = reference(engines, "small", SMALL)
    n = SMALL["n"]
    batch = SegBatch(engines)
    frags = [torch.from_numpy(r["frags"]).cuda() for r in refs]
    bad = 1
    assert int(refs[bad]["graph"][3][0]) > 8
    bufs = [graph_buffers(8 if i == bad else EDGE_CAP) for i in range(n)]
    batch.rag_graph(affs, frags, *[list(x) for x in zip(*bufs)])
    for i, e in enumerate(engines):
        if i == bad:
            with pytest.raises(_lib.BsmiError) as exc:
                e.status()
            assert exc.value.code == _lib.ERR_OVERFLOW and "flags 0x20" in str(exc.value)
            assert int(bufs[i][3][0]) == int(refs[i]["graph"][3][0])   # the number of edges the block needs
        else:
            e.status()
            check_graph(refs[i], sorted_graph(*bufs[i]))
    bufs = [graph_buffers(EDGE_CAP) for _ in range(n)]
    batch.rag_graph(affs, frags, *[list(x) for x in zip(*bufs)])
    for i, e in enumerate(engines):
        e.status()
        check_graph(refs[i], sorted_graph(*bufs[i]))


def test_slices_off_the_lds_path_are_refused():
    from bootstrapper_amd import _lib
    from bootstrapper_amd.post.engine import SegBatch, SegEngine
    shape = (3, 200, 300)
    engs = [SegEngine(shape, 0) for _ in range(2)]
    batch = SegBatch(engs)
    affs = [torch.zeros((3,) + shape, dtype=torch.uint8, device="cuda") for _ in range(2)]
    case = dict(shape=shape, crop_offset=(1, 8, 8))
    with pytest.raises(_lib.BsmiError) as exc:
        batched_fragments(batch, affs, case, [0, 1])
    assert exc.value.code == _lib.ERR_INVALID and "LDS" in str(exc.value)
    fr = [torch.zeros(shape, dtype=torch.int64, device="cuda") for _ in range(2)]
    bufs = [graph_buffers(64) for _ in range(2)]
    with pytest.raises(_lib.BsmiError) as exc:
        batch.rag_graph(affs, fr, *[list(x) for x in zip(*bufs)])
    assert exc.value.code == _lib.ERR_INVALID
    for e in engs:
        e.status()


def run_slab(monkeypatch, batch, shape, block, ctx, lanes, affs):
    from bootstrapper_amd.volume import SlabSegmenter
    monkeypatch.setenv("BSMI_SEG_BATCH", "1" if batch else "0")
    thr = [0.3, 0.45]
    seg = SlabSegmenter(shape, block, ctx, -(-shape[0] // block[0]), 0, thr, True, MSD, FILT, DEBRIS, 256, n_lanes=lanes)
    assert bool(seg._batchers) == batch
    refused = []
    if batch:
        stage = seg._batch_stage

        def spy(kind, ks, wait=()):
            r = stage(kind, ks, wait)
            refused.append((len(ks), len(r)))
            return r
        seg._batch_stage = spy
    seg.interior(seg.affs).copy_(torch.from_numpy(affs).cuda())
    segs = seg.run()
    o = np.lexsort((seg.rag_edges[:, 1], seg.rag_edges[:, 0]))
    ids, pos, size = seg.node_table()
    return dict(frags=seg.interior(seg.frags).cpu().numpy(), nodes=seg.nodes, edges=seg.rag_edges[o], scores=seg.rag_scores[o],
                segs=segs.cpu().numpy(), pos=pos, size=size), refused


def same(a, b):
    assert len(a["nodes"]) > 20 and len(a["edges"]) > 20
    for key in a:
        assert np.array_equal(a[key], b[key]), key


def test_pipeline_in_batches_equals_the_lanes(monkeypatch):
    """ragged blocks (several read shapes) and more blocks than workspaces (several batches per shape)"""
    shape, block, ctx = (20, 150, 130), (8, 64, 64), (1, 8, 8)
    affs = blobby(shape, 21)
    affs[:, :, :40, :50] = 0
    got, refused = run_slab(monkeypatch, True, shape, block, ctx, 5, affs)
    ref, _ = run_slab(monkeypatch, False, shape, block, ctx, 5, affs)
    assert refused == [(27, 0), (27, 0)]   # every block of both stages went through the batches
    same(got, ref)


def test_pipeline_takes_the_lanes_for_refused_shapes(monkeypatch):
    shape, block, ctx = (2, 368, 568), (1, 184, 284), (1, 8, 8)   # read boxes of (3, 200, 300)
    affs = blobby(shape, 5)
    got, refused = run_slab(monkeypatch, True, shape, block, ctx, 3, affs)
    ref, _ = run_slab(monkeypatch, False, shape, block, ctx, 3, affs)
    assert refused == [(8, 8), (8, 8)]
    same(got, ref)
