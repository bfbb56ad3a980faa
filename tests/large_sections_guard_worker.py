"""Worker of tests/test_large_sections_gpu.py: with BSMI_GUARD_MB set, every device allocation of the segmentation engine lies
between zones of 0xFF bytes; fragments of two 1250 x 1250 sections (the wide flood and its HBM spill), their agglomeration
-> zones written to (0), results equal to the oracle."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from scipy.ndimage import gaussian_filter
from bootstrapper_amd import _lib
from bootstrapper_amd.post.engine import SegEngine
from oracle import seg_ref as S

assert os.environ.get("BSMI_GUARD_MB")
rng = np.random.default_rng(5)
a = gaussian_filter(rng.random((3, 2, 1250, 1250), dtype=np.float32), sigma=(0, 0, 6, 6))
affs = ((a - a.min()) / (a.max() - a.min()) * 255).astype(np.uint8)
eng = SegEngine(affs.shape[1:], 0)
t = torch.from_numpy(affs).cuda()
frags, mx = eng.ws_fragments(t, True, 10)
segs = eng.agglomerate_mean(t, frags, [0.2, 0.5])
eng.status()
torch.cuda.synchronize()
bad = _lib.lib.bsmi_debug_check_guards()
assert bad == 0, f"{bad} guard zones written to"
ref, ref_max = S.ws_fragments_u8(affs, True, 10)
assert int(mx.item()) == ref_max and np.array_equal(frags.cpu().numpy().astype(np.uint64), ref)
for s, r in zip(segs, S.agglomerate_mean_u8(affs, ref, [0.2, 0.5])):
    assert np.array_equal(s.cpu().numpy().astype(np.uint64), r)
print("guards intact", flush=True)
