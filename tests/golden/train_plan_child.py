"""One pass (and its repeat) over the grid of make_train_plan_fixture.py on the GPU, at the head counts of the named setting and under
the experiment switches of this process's environment:

    python tests/golden/train_plan_child.py SETTING OUT.npz

Per point: gnngls_profile_enable(1), the training forward, the backward, gnngls_profile_collect; the spans per kind and the SHA-256
of the bytes of y_out, bn_batch_stats and the gradient image are recorded, the arrays themselves for the points of KEPT / KEPT_GRADS.
Every output must be finite and the second pass must repeat every span and digest.  Run by the fixture maker and by
test_train_plan_gpu.py as a fresh process per setting; any failure is a non-zero exit."""
import ctypes
import hashlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_train_plan_fixture as mt  # noqa: E402

from gnngls_amd import _lib  # noqa: E402

SENTINEL = -7.0      # what the outputs hold before the call


def main(setting, out_path):
    L = _lib.load()
    dev = torch.device("cuda")
    heads = dict((name, h) for name, _, h in mt.SETTINGS)[setting]
    all_pts = mt.grid_points()
    index = [i for i, p in enumerate(all_pts) if p[1] in heads]
    pts = [all_pts[i] for i in index]
    params, feats = {}, {}
    vp = ctypes.c_void_p

    def params_of(in_dim, layers):
        if (in_dim, layers) not in params:
            rng = np.random.default_rng(1000 * in_dim + layers)
            w = (rng.standard_normal(L.gnngls_model_packed_floats(in_dim, layers)) * 0.05).astype(np.float32)
            params[in_dim, layers] = torch.from_numpy(w).to(dev)
        return params[in_dim, layers]

    def data_of(n, B, in_dim):
        if (n, B, in_dim) not in feats:
            rng = np.random.default_rng(100000 * n + 100 * in_dim + B)
            x = rng.random((B, mt.pairs(n), in_dim), dtype=np.float32)
            dy = rng.standard_normal((B, mt.pairs(n))).astype(np.float32)
            feats[n, B, in_dim] = torch.from_numpy(x).to(dev), torch.from_numpy(dy).to(dev)
        return feats[n, B, in_dim]

    ms = (ctypes.c_double * mt.N_PROF_KINDS)()
    cnt = (ctypes.c_int64 * mt.N_PROF_KINDS)()

    def one_pass(keep):
        spans = np.zeros((len(pts), len(mt.KINDS)), np.int16)
        digests = np.zeros((len(pts), len(mt.WHAT), 32), np.uint8)
        kept = {}
        for i, p in enumerate(pts):
            n, H, layers, in_dim, B = p
            N = mt.pairs(n)
            ws_bytes = L.gnngls_regret_train_workspace_bytes_heads(B, n, layers, H)
            ws = torch.zeros(ws_bytes, dtype=torch.uint8, device=dev)
            w, (x, dy) = params_of(in_dim, layers), data_of(n, B, in_dim)
            y = torch.full((B * N,), SENTINEL, dtype=torch.float32, device=dev)
            stats = torch.full((max(layers, 1) * 4 * 128,), SENTINEL, dtype=torch.float32, device=dev)
            grads = torch.full((w.numel(),), SENTINEL, dtype=torch.float32, device=dev)
            st = _lib.current_stream()
            _lib.check(L.gnngls_profile_enable(1), "profile_enable")
            _lib.check(L.gnngls_regret_train_forward_heads(vp(x.data_ptr()), vp(w.data_ptr()), B, n, in_dim, layers, H, mt.BN_EPS,
                                                           vp(y.data_ptr()), vp(stats.data_ptr()), vp(ws.data_ptr()), ws_bytes, st),
                       f"train_forward at {p}")
            _lib.check(L.gnngls_regret_train_backward_heads(vp(x.data_ptr()), vp(w.data_ptr()), vp(dy.data_ptr()), B, n, in_dim, layers, H,
                                                            vp(grads.data_ptr()), vp(ws.data_ptr()), ws_bytes, st), f"train_backward at {p}")
            _lib.check(L.gnngls_profile_collect(ctypes.cast(ms, vp), ctypes.cast(cnt, vp)), "profile_collect")
            torch.cuda.synchronize()
            arrays = [y.cpu().numpy(), stats.cpu().numpy()[:layers * 4 * 128], grads.cpu().numpy()]
            for what, a in zip(mt.WHAT, arrays):
                assert np.isfinite(a).all(), f"{what} is not finite at {p}"
            spans[i] = [cnt[k] for k in mt.KIND_INDEX]
            assert sum(cnt) == spans[i].sum(), f"a span of another kind at {p}"
            digests[i] = [np.frombuffer(hashlib.sha256(a.tobytes()).digest(), np.uint8) for a in arrays]
            if keep and p in mt.KEPT:
                kept[f"y{mt.KEPT.index(p)}"], kept[f"stats{mt.KEPT.index(p)}"] = arrays[0].copy(), arrays[1].copy()
            if keep and p in mt.KEPT_GRADS:
                kept[f"grads{mt.KEPT_GRADS.index(p)}"] = arrays[2].copy()
        _lib.check(L.gnngls_profile_enable(0), "profile_enable")
        return spans, digests, kept

    spans, digests, kept = one_pass(True)
    spans2, digests2, _ = one_pass(False)
    bad = np.argwhere((digests != digests2).any(axis=(1, 2)) | (spans != spans2).any(axis=1)).reshape(-1)
    assert bad.size == 0, f"the second pass differs at {len(bad)} points: {[pts[int(b)] for b in bad[:20]]}"
    assert setting != mt.SETTINGS[0][0] or len(kept) == 2 * len(mt.KEPT) + len(mt.KEPT_GRADS)
    np.savez(out_path, index=np.asarray(index, np.int32), spans=spans, digests=digests, **kept)
    print("train_plan_child:", setting, len(pts), "points,", {k: os.environ[k] for k in mt.SWITCH_VARS if k in os.environ})


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
