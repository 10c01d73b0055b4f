"""Batched end-to-end hot path: the body of the reference's per-instance loop (scripts/test.py:59-104)
for B independent instances at once, entirely on the GPU.

    features (datasets.py:73-95) -> model forward (test.py:76-77) -> inverse scaler + clamp
    (test.py:79-83) -> start tour on the guide: nearest_neighbor (test.py:85) or an insertion constructor
    (algorithms.py:82-108) -> tour_cost (test.py:90)
    -> guided_local_search with the remaining budget (test.py:91-95)

The 10 s budget of the reference starts before the forward pass (test.py:64), so the search gets
`time_limit - elapsed`.  At most `gls_resident_capacity(n)` instances are searched concurrently (one
persistent workgroup each); larger batches are processed in chunks, each with its own budget.

Multi-start (`starts=R > 1`): every instance is searched R times in the same launch -- run 0 from the start tour above, runs
1..R-1 from sampled nearest-neighbour walks on the distances (ops.sample_nn_tours, invert=True) -- and the first run with the
smallest cost is the instance's result.  A chunk then holds capacity // R instances: a batch that leaves search slots idle
fills them with further runs of its own instances instead.
"""
import dataclasses
import time
import warnings
from dataclasses import dataclass, field

import torch

from . import models as M
from . import ops


@dataclass
class Scalers:
    """MinMaxScaler parameters (sklearn: transform = x*scale_ + min_), datasets.py:48-51."""
    feat_scale: float
    feat_min: float
    regret_scale: float = 1.0
    regret_min: float = 0.0

    @staticmethod
    def from_sklearn(scalers):
        if "edges" in scalers:            # backward compatibility, datasets.py:48-49
            scalers = scalers["edges"]
        f, r = scalers["features"], scalers["regret"]
        return Scalers(float(f.scale_[0]), float(f.min_[0]), float(r.scale_[0]), float(r.min_[0]))

    @staticmethod
    def fit_weights(D):
        """MinMax scaler fitted on the off-diagonal weights of a batch (synthetic substitute for
        preprocess_dataset.py:39-48); regret scaler = identity (data_min 0, data_max 1)."""
        n = D.shape[-1]
        mask = ~torch.eye(n, dtype=torch.bool, device=D.device)
        w = D[..., mask].float().double()
        lo, hi = w.min().item(), w.max().item()
        scale = 1.0 / (hi - lo)
        return Scalers(scale, 0.0 - lo * scale, 1.0, 0.0)


@dataclass
class SolveResult:
    best_tour: torch.Tensor
    best_cost: torch.Tensor
    init_cost: torch.Tensor
    outer_iters: torch.Tensor
    evals: torch.Tensor
    moves: torch.Tensor
    status: torch.Tensor
    regret_pred: torch.Tensor = None
    timing: dict = field(default_factory=dict)
    trace_cost: torch.Tensor = None
    trace_time: torch.Tensor = None
    # bounded improvement record (the returned best whenever it improved, ops.GlsResult) and the host clock
    imp_cost: torch.Tensor = None
    imp_time: torch.Tensor = None
    imp_iter: torch.Tensor = None
    imp_len: torch.Tensor = None
    evals_executed: torch.Tensor = None   # [B] int64, only with count_executed (measurement hook, ops.executed_evals)
    start_time: torch.Tensor = None    # [B] fp64 host time.time() at which the instance's budget started (test.py:64)
    launch_time: torch.Tensor = None   # [B] fp64 host time.time() just before its search kernel was launched
    # only with lower_bound=True: the Held-Karp 1-tree bound of every instance (ops.one_tree_bound with ub = best_cost), a
    # certified lower_bound <= optimum <= best_cost, and how its ascent ended (ops.BOUND_EXIT_*; TOUR: the bound is the optimum)
    lower_bound: torch.Tensor = None   # [B] fp64
    bound_exit: torch.Tensor = None    # [B] int32
    # only with starts = R > 1: the returned cost of every run (run 0 = the start tour `init`) and the run whose result the other
    # per-instance fields carry: the first with the smallest cost
    start_costs: torch.Tensor = None   # [B,R] fp64
    best_start: torch.Tensor = None    # [B] int64
    # only with polish="or_opt": best_cost before the polishing descent minus best_cost after it, >= 0 (best_tour / best_cost are
    # the polished ones)
    polish_gain: torch.Tensor = None   # [B] fp64
    polish_time: torch.Tensor = None   # [B] fp64 host time.time() at which the polish of the instance's chunk ended


# start tours of solve_batch -> mode of ops.insertion (None: ops.nearest_neighbor)
INIT_TOURS = {"nearest_neighbor": None, "nearest_insertion": "nearest", "farthest_insertion": "farthest"}


def predict_regret(model, D, scalers, features=None):
    """-> 'regret_pred' guide matrices [B,n,n] fp64 (test.py:72-83).
    features: None = the reference's default feature set, the scaled edge weight (datasets.py:14-20 set_features), packed
    from D on the device; else a [B, N, in_dim] fp32 tensor of ALREADY scaled features in line-graph node order
    (TSPDataset.get_scaled_features: any feature set, after `feat_drop_idx`), fed to the forward as it is."""
    B, n, _ = D.shape
    if features is None:
        feat = M.pack_features(D, scalers.feat_scale, scalers.feat_min)
    else:
        N = n * (n - 1) // 2
        assert features.dtype == torch.float32 and features.shape[:2] == (B, N) and features.shape[2] == model.in_dim
        feat = features.to(D.device).reshape(B * N, model.in_dim).contiguous()
    y = M.regret_forward(model, feat, B, n)
    return M.unpack_regret(y, n, scalers.regret_scale, scalers.regret_min)


def solve_batch(D, model=None, scalers=None, guides=("regret_pred",), time_limit=10.0, perturbation_moves=20,
                first_improvement=False, max_outer_iters=-1, trace_cap=0, want_trace_time=False, chunk=None,
                keep_regret=False, budget="per_instance", imp_cap=0, features=None, count_executed=False,
                init="nearest_neighbor", init_weight="auto", lower_bound=False, bound_iters=2000, starts=1, start_seed=0,
                alpha_iters=2000, polish=None, polish_seg=3):
    """D [B,n,n] fp64 CUDA tensor (symmetric).  Returns SolveResult with per-instance tensors.

    budget="per_instance" (default, the reference's meaning of --time_limit, test.py:64,92): every instance is searched
    for `time_limit` seconds; a batch larger than the device capacity takes ceil(B/capacity) rounds of `time_limit` each.
    budget="per_batch": the whole batch finishes within `time_limit`; the rounds share it equally (each instance is
    searched for time_limit / rounds) -- the throughput end of the same trade, with the gap there to judge it.
    features: see predict_regret (None = scaled edge weights packed on the device).
    count_executed: also return the delta evaluations the search kernel actually executed (bench.py's roofline).
    init: the start tour -- "nearest_neighbor" (test.py:85), "nearest_insertion" or "farthest_insertion" (the reference's
    insertion(G, depot, mode), algorithms.py:82-108), from depot 0.
    init_weight: the matrix the start tour is built on.  "auto" keeps the reference's rule (test.py:70-88: 'regret_pred'
    whenever that guide is used at all, else 'weight'); "weight" builds it on the distances even when the model guides the search.
    lower_bound: after a chunk's search has ended (outside its budget) also compute the Held-Karp 1-tree bound of its instances
    with at most `bound_iters` 1-trees and ub = best_cost -> SolveResult.lower_bound, .bound_exit and timing["bound_s"].
    starts: R > 1 searches every instance R times in one launch (run 0 from `init`, runs 1..R-1 from sampled walks on D keyed by
    `start_seed` and the instance's index in the batch, so chunking does not change them) and returns the first run with the
    smallest cost; a chunk holds capacity // R instances.  SolveResult.start_costs [B,R], .best_start [B], timing["sample_s"]
    (the one sampling launch of the batch; its time is taken off the rounds' budgets in equal shares).
    guides: any mix and order of 'regret_pred' (the model), 'weight' (the distances) and 'alpha' -- Helsgaun's alpha-nearness
    (ops.alpha_nearness), computed per chunk inside its budget like the forward: the Held-Karp ascent of ops.one_tree_bound with
    ub = the nearest-neighbour tour's length on the distances and at most `alpha_iters` 1-trees gives the potentials
    (alpha_iters=0: no ascent, zero potentials), one more launch the matrix; its time goes to timing["alpha_s"] (absent when the
    guide is unused).  It needs no model.  The start tour keeps the reference's rule whatever 'alpha' does: alpha is zero on the n
    edges of the minimum 1-tree of every instance and is no matrix to walk greedily.  alpha_iters defaults to bound_iters'
    default, the oracle's 2000: measured (profiles/alpha_guide.json) it gives the best alpha guide wherever the budget is three
    times the ascent's time or more (0.13 s for 1,024 TSP100, 0.35 s for 256 TSP200 instances); under a shorter budget lower it.
    polish: "or_opt" runs ops.or_opt_descent (2-opt and Or-opt with chains of up to `polish_seg` nodes, reversal on, the default
    move cap) on the returned best tours after a chunk's search has ended, outside its budget as lower_bound is (with starts > 1
    on the winner only; with lower_bound before the bound, so that ub is the polished cost).  The polished tours and costs replace
    best_tour and best_cost; SolveResult.polish_gain [B] = cost before - cost after >= 0, .polish_time, timing["polish_s"].
    None (default): today's call sequence, polish_gain None, no timing key."""
    if init not in INIT_TOURS:
        raise ValueError(f"unknown start tour {init!r} (one of {', '.join(INIT_TOURS)})")
    if init_weight not in ("auto", "weight"):
        raise ValueError(f"unknown init_weight {init_weight!r} ('auto' or 'weight')")
    insert_mode = INIT_TOURS[init]
    if polish not in (None, "or_opt"):
        raise ValueError(f"unknown polish {polish!r} (None or 'or_opt')")
    polish_seg = int(polish_seg)
    if polish is not None and not 1 <= polish_seg <= ops.OR_OPT_MAX_SEG:
        raise ValueError(f"polish_seg={polish_seg} must be in 1..{ops.OR_OPT_MAX_SEG}")
    starts = int(starts)
    if starts < 1:
        raise ValueError(f"starts={starts} must be >= 1")
    if budget not in ("per_instance", "per_batch"):
        raise ValueError(f"unknown budget policy {budget!r}")
    assert D.is_cuda and D.dtype == torch.float64
    B, n, _ = D.shape
    guides = list(guides)
    need_model = "regret_pred" in guides
    need_alpha = "alpha" in guides
    alpha_iters = int(alpha_iters)
    if need_alpha and alpha_iters < 0:
        raise ValueError(f"alpha_iters={alpha_iters} must be >= 0")
    if need_model and (model is None or scalers is None):
        raise ValueError("guide 'regret_pred' needs a model and scalers")
    for g in guides:
        if g not in ("regret_pred", "weight", "alpha"):
            raise ValueError(f"unknown guide {g!r}")
    if B == 0:                            # an empty shard (more ranks than instances): nothing to launch
        e64 = torch.zeros((0,), dtype=torch.float64, device=D.device)
        ei64, ei32 = e64.long(), e64.int()
        return SolveResult(best_tour=torch.zeros((0, n + 1), dtype=torch.int32, device=D.device), best_cost=e64,
                           init_cost=e64, outer_iters=ei64, evals=ei64, moves=ei32, status=ei32,
                           timing={"forward_s": 0.0, "init_s": 0.0, "search_s": 0.0, "chunks": 0},
                           start_time=e64.cpu(), launch_time=e64.cpu(), lower_bound=e64 if lower_bound else None,
                           bound_exit=ei32 if lower_bound else None,
                           start_costs=e64.reshape(0, starts) if starts > 1 else None, best_start=ei64 if starts > 1 else None,
                           polish_gain=e64 if polish else None, polish_time=e64.cpu() if polish else None)
    cap = ops.gls_resident_capacity(n)
    if chunk is None:
        chunk = max((cap if cap > 0 else 64) // starts, 1)
        # equal-sized rounds: a batch a little larger than the device capacity is split evenly (same number of
        # rounds, i.e. the same wall time, but every round leaves the SIMDs less crowded)
        rounds = -(-B // chunk)
        chunk = -(-B // rounds) if B > 0 else chunk
    outs, timing = [], {"forward_s": 0.0, "init_s": 0.0, "search_s": 0.0, "chunks": 0}
    n_rounds = -(-B // chunk) if B > 0 else 1
    round_limit = time_limit / n_rounds if budget == "per_batch" else time_limit
    sampled, sample_s = None, 0.0
    if starts > 1:
        ts = time.time()
        sampled, _ = ops.sample_nn_tours(D, starts - 1, 0, True, start_seed)      # [B,R-1,n+1]: walk (b, r) belongs to instance b
        torch.cuda.synchronize()
        sample_s = time.time() - ts
        timing["sample_s"] = sample_s
    for b0 in range(0, B, chunk):
        Dc = D[b0:b0 + chunk].contiguous()
        t0 = time.time()                                                   # test.py:64
        R = None
        if need_model:
            R = predict_regret(model, Dc, scalers, None if features is None else features[b0:b0 + chunk])
            torch.cuda.synchronize()
        t1 = time.time()
        A = None
        if need_alpha:
            pi = None
            if alpha_iters > 0:
                ub = ops.tour_cost(ops.nearest_neighbor(Dc), Dc)
                pi = ops.one_tree_bound(Dc, ub, max_iters=alpha_iters).pi
            A = ops.alpha_nearness(Dc, pi)
            torch.cuda.synchronize()
            timing["alpha_s"] = timing.get("alpha_s", 0.0) + (time.time() - t1)
        t1a = time.time()
        # test.py:70-88: the start tour is greedy on 'regret_pred' whenever that guide is used AT ALL (not only when it
        # comes first), otherwise on 'weight'
        Wi = R if (need_model and init_weight == "auto") else Dc
        # the defaults give nearest_neighbor(R if need_model else Dc): the call this function always made
        init = ops.nearest_neighbor(Wi) if insert_mode is None else ops.insertion(Wi, 0, insert_mode)
        init_cost = ops.tour_cost(init, Dc)                                # test.py:90
        gt = torch.stack([{"regret_pred": R, "weight": Dc, "alpha": A}[g] for g in guides]).contiguous()
        Ds = Dc
        if starts > 1:
            # job c * starts + r = run r of instance c: the matrices are replicated per run, the start tours interleaved
            init = torch.cat([init[:, None], sampled[b0:b0 + chunk]], dim=1).reshape(-1, n + 1).contiguous()
            Ds = Dc.repeat_interleave(starts, dim=0)
            gt = gt.repeat_interleave(starts, dim=1)
            init_cost = ops.tour_cost(init, Ds)
        torch.cuda.synchronize()
        t2 = time.time()
        remaining = max(round_limit - (t2 - t0) - sample_s / n_rounds, 0.0)
        run = lambda: ops.gls_run(Ds, gt, init, init_cost, perturbation_moves=perturbation_moves,   # noqa: E731
                                  first_improvement=first_improvement, max_outer_iters=max_outer_iters,
                                  time_limit_s=remaining, trace_cap=trace_cap, want_trace_time=want_trace_time, imp_cap=imp_cap)
        executed = None
        if count_executed:
            with ops.executed_evals(Ds.shape[0]) as x:
                r = run()
            executed = x.counts
            timing["cycle_records"] = [x.record(Ds.shape[0], k).clone() for k in range(1, ops.EXEC_RECORDS)]     # of the last device load
        else:
            r = run()
        torch.cuda.synchronize()
        t3 = time.time()
        aborted = int((r.status == ops.STATUS_WATCHDOG).sum())
        if aborted:
            warnings.warn(f"solve_batch: the device watchdog stopped {aborted} search(es) early (best-so-far returned)",
                          RuntimeWarning, stacklevel=2)
        timing["forward_s"] += t1 - t0
        timing["init_s"] += t2 - t1a
        timing["search_s"] += t3 - t2
        timing["chunks"] += 1
        start_costs = best_start = None
        if starts > 1:
            start_costs = r.best_cost.reshape(-1, starts).clone()
            best_start = ops.first_argmin(start_costs)
            win = torch.arange(Dc.shape[0], device=D.device) * starts + best_start
            r = dataclasses.replace(r, **{f.name: getattr(r, f.name)[win] for f in dataclasses.fields(r)
                                          if getattr(r, f.name) is not None})
            init_cost = init_cost[win]
            if executed is not None:
                executed = executed[win]
        gain = polish_end = None
        if polish:
            tp = time.time()
            po = ops.or_opt_descent(r.best_tour.contiguous(), r.best_cost.contiguous(), Dc, polish_seg, True)
            gain = r.best_cost - po.cost
            r = dataclasses.replace(r, best_tour=po.tour, best_cost=po.cost)
            torch.cuda.synchronize()
            polish_end = torch.full((Dc.shape[0],), time.time(), dtype=torch.float64)
            timing["polish_s"] = timing.get("polish_s", 0.0) + (float(polish_end[0]) - tp)
        lb = None
        if lower_bound:
            tb = time.time() if polish else t3
            lb = ops.one_tree_bound(Dc, r.best_cost, max_iters=bound_iters, want_pi=False)
            torch.cuda.synchronize()
            timing["bound_s"] = timing.get("bound_s", 0.0) + (time.time() - tb)
        outs.append((r, init_cost, R if keep_regret else None,
                     torch.full((Dc.shape[0],), t0, dtype=torch.float64), torch.full((Dc.shape[0],), t2, dtype=torch.float64),
                     executed, lb, start_costs, best_start, gain, polish_end))
    cat = lambda xs: torch.cat(xs) if len(xs) > 1 else xs[0]  # noqa: E731
    return SolveResult(
        best_tour=cat([o[0].best_tour for o in outs]), best_cost=cat([o[0].best_cost for o in outs]),
        init_cost=cat([o[1] for o in outs]), outer_iters=cat([o[0].outer_iters for o in outs]),
        evals=cat([o[0].evals for o in outs]), moves=cat([o[0].trace_len for o in outs]),
        status=cat([o[0].status for o in outs]),
        regret_pred=cat([o[2] for o in outs]) if keep_regret and need_model else None, timing=timing,
        trace_cost=cat([o[0].trace_cost for o in outs]) if trace_cap > 0 else None,
        trace_time=cat([o[0].trace_time for o in outs]) if (trace_cap > 0 and want_trace_time) else None,
        imp_cost=cat([o[0].imp_cost for o in outs]) if imp_cap > 0 else None,
        imp_time=cat([o[0].imp_time for o in outs]) if imp_cap > 0 else None,
        imp_iter=cat([o[0].imp_iter for o in outs]) if imp_cap > 0 else None,
        imp_len=cat([o[0].imp_len for o in outs]) if imp_cap > 0 else None,
        evals_executed=cat([o[5] for o in outs]) if count_executed else None,
        start_time=cat([o[3] for o in outs]), launch_time=cat([o[4] for o in outs]),
        lower_bound=cat([o[6].bound for o in outs]) if lower_bound else None,
        bound_exit=cat([o[6].exit_kind for o in outs]) if lower_bound else None,
        start_costs=cat([o[7] for o in outs]) if starts > 1 else None,
        best_start=cat([o[8] for o in outs]) if starts > 1 else None,
        polish_gain=cat([o[9] for o in outs]) if polish else None,
        polish_time=cat([o[10] for o in outs]) if polish else None)


def synthetic_model(seed=1234, device="cuda"):
    """Seeded synthetic checkpoint with the reference architecture (embed 128, 8 heads, 8 layers --
    models.py:59-61) and non-trivial BatchNorm statistics (the reference's checkpoints are LFS stubs)."""
    torch.manual_seed(seed)
    model = M.EdgePropertyPredictionModel(1, 128, 1, 3, n_heads=8)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for mod in model.modules():
            if isinstance(mod, torch.nn.BatchNorm1d):
                mod.running_mean.copy_(0.1 * torch.randn(mod.running_mean.shape, generator=g))
                mod.running_var.copy_(0.5 + torch.rand(mod.running_var.shape, generator=g))
                mod.weight.copy_(1.0 + 0.1 * torch.randn(mod.weight.shape, generator=g))
                mod.bias.copy_(0.1 * torch.randn(mod.bias.shape, generator=g))
    return model.eval().to(device)
