"""One pass (and its repeat) over the accepted points of make_forward_plan_fixture.py on the GPU, under the experiment switches of
this process's environment:

    python tests/golden/forward_plan_child.py OUT.npz

Per point: gnngls_profile_enable(1), the forward, gnngls_profile_collect; the spans per kind and the SHA-256 of y_out's bytes are
recorded, y_out itself for the points of KEPT.  Every y_out must be finite and the second pass must repeat every digest.  Run by the
fixture maker and by test_forward_plan_gpu.py as a fresh process per switch setting; any failure is a non-zero exit."""
import ctypes
import hashlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_forward_plan_fixture as mk  # noqa: E402

from gnngls_amd import _lib  # noqa: E402


def main(out_path):
    L = _lib.load()
    dev = torch.device("cuda")
    pts = mk.accepted_points()
    weights, images, feats = {}, {}, {}
    vp = ctypes.c_void_p

    def weights_of(in_dim, layers):
        if (in_dim, layers) not in weights:
            rng = np.random.default_rng(1000 * in_dim + layers)
            w = (rng.standard_normal(L.gnngls_model_packed_floats(in_dim, layers)) * 0.05).astype(np.float32)
            weights[in_dim, layers] = torch.from_numpy(w).to(dev)
        return weights[in_dim, layers]

    def image_of(in_dim, layers, H):
        if (in_dim, layers, H) not in images:
            img = torch.zeros(L.gnngls_regret_prepared_bytes(layers), dtype=torch.uint8, device=dev)
            _lib.check(L.gnngls_regret_prepare_heads(vp(weights_of(in_dim, layers).data_ptr()), in_dim, layers, H, vp(img.data_ptr()),
                                                     img.numel(), _lib.current_stream()), "regret_prepare_heads")
            images[in_dim, layers, H] = img
        return images[in_dim, layers, H]

    def feat_of(n, B, in_dim):
        if (n, B, in_dim) not in feats:
            rng = np.random.default_rng(100000 * n + 100 * in_dim + B)
            feats[n, B, in_dim] = torch.from_numpy(rng.random((B, mk.pairs(n), in_dim), dtype=np.float32)).to(dev)
        return feats[n, B, in_dim]

    ms = (ctypes.c_double * mk.N_PROF_KINDS)()
    cnt = (ctypes.c_int64 * mk.N_PROF_KINDS)()

    def one_pass(keep):
        spans = np.zeros((len(pts), len(mk.KINDS)), np.int16)
        digests = np.zeros((len(pts), 32), np.uint8)
        kept = {}
        for i, p in enumerate(pts):
            n, H, layers, in_dim, form, bmode = p
            B, N = mk.batch_of(bmode), mk.pairs(n)
            ws_bytes = L.gnngls_regret_forward_workspace_bytes_heads(2 if bmode == 1 else B, n, H)
            store = torch.empty(ws_bytes + 512, dtype=torch.uint8, device=dev)
            ws_ptr = ((store.data_ptr() + 255) & ~255) + (4 if bmode == 2 else 0)
            w, x = weights_of(in_dim, layers), feat_of(n, B, in_dim)
            y = torch.full((B, N), float("nan"), dtype=torch.float32, device=dev)
            image = image_of(in_dim, layers, H) if form == mk.FORM_PREPARED else None
            st = _lib.current_stream()
            _lib.check(L.gnngls_profile_enable(1), "profile_enable")
            if form == mk.FORM_ONE_CALL:
                rc = L.gnngls_regret_forward_heads(vp(x.data_ptr()), vp(w.data_ptr()), B, n, in_dim, layers, H, vp(y.data_ptr()),
                                                   vp(ws_ptr), ws_bytes, st)
            else:
                rc = L.gnngls_regret_forward_prepared_heads(vp(x.data_ptr()), vp(w.data_ptr()), vp(image.data_ptr()) if image is not None else None,
                                                            image.numel() if image is not None else 0, B, n, in_dim, layers, H,
                                                            vp(y.data_ptr()), vp(ws_ptr), ws_bytes, st)
            _lib.check(rc, f"forward at {p}")
            _lib.check(L.gnngls_profile_collect(ctypes.cast(ms, vp), ctypes.cast(cnt, vp)), "profile_collect")
            torch.cuda.synchronize()
            yh = y.cpu().numpy()
            assert np.isfinite(yh).all(), f"y_out is not finite at {p}"
            spans[i] = [cnt[k] for k in mk.KIND_INDEX]
            assert sum(cnt) == spans[i].sum(), f"a span of another kind at {p}"
            digests[i] = np.frombuffer(hashlib.sha256(yh.tobytes()).digest(), np.uint8)
            if keep and p in mk.KEPT:
                kept[mk.KEPT.index(p)] = yh.reshape(-1).copy()
        _lib.check(L.gnngls_profile_enable(0), "profile_enable")
        return spans, digests, kept

    spans, digests, kept = one_pass(True)
    spans2, digests2, _ = one_pass(False)
    bad = np.argwhere((digests != digests2).any(axis=1) | (spans != spans2).any(axis=1)).reshape(-1)
    assert bad.size == 0, f"the second pass differs at {len(bad)} points, first {pts[int(bad[0])]}"
    assert len(kept) == len(mk.KEPT)
    np.savez(out_path, points=np.asarray(pts, np.int16), spans=spans, digests=digests, **{f"y{k}": v for k, v in kept.items()})
    print("forward_plan_child:", len(pts), "points,", {k: os.environ[k] for k in mk.SWITCH_VARS if k in os.environ})


if __name__ == "__main__":
    main(sys.argv[1])
