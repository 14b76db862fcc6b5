"""Host-side drivers above the C ABI: the benchmark configurations of BASELINE.json, the panorama chain of
ImageProcess::matching (ImageProcess.cpp:159-268, hot-path calls only; from features alone: panorama_from_features), and the sharding of independent pairs
across the GPUs of a node (one process per GPU, torch.distributed; backend "nccl" is RCCL over xGMI).

Nothing here computes pixels: every per-pixel operation is a HIP kernel reached through capi.
"""
import math

import numpy as np

from . import capi

SEED_MAP = (1.0, 0.002, 1e-6, -2048.0, -0.001, 1.0, 5e-7, 1.5)  # config-2 backward map, SURVEY.md 8(d)


def config_map(pair_index=0, frame=4096):
    """Backward map of synthetic pair `pair_index`: p[3] = -(frame/2) - 8*i so that pairs differ (config 4)."""
    p = list(SEED_MAP)
    p[3] = -(frame / 2.0) - 8.0 * pair_index
    return p


def config_canvas(frame=4096):
    """Canvas of the synthetic pair configs: fixed by definition at 1.5*frame x frame (6144x4096 for config 2)."""
    return frame * 3 // 2, frame


def shard_range(n_items, rank, world):
    """Contiguous shard [lo, hi) of n_items for `rank` (config 4: 32 pairs -> 4 per GPU on 8 ranks)."""
    base, rem = divmod(n_items, world)
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)


def algorithmic_bytes(frame_px_a, frame_px_b, level_w, level_h, bytes_per_sample=4, fused_sweep_levels=0, fused_decimate=True,
                      source_fused=False, implicit_mask=False, coarse_from=0):
    """SURVEY.md 8(d) byte accounting for one pair: every distinct input array read once + every output array
    written once, pyramid planes f32.  Returns (per_kernel, stages): `stages` are the canonical totals S1..S3 the
    headline fraction uses (independent of how the kernels are fused); `per_kernel` gives each of THIS implementation's
    kernels the bytes it actually owns -- its own inputs read once and its own outputs written once, given the fusion
    the plan runs with -- so that no kernel is credited traffic another kernel (or nobody) moves:
      fused_decimate   k_vv_y_bwd_dec reads level l and writes only level l+1 (the blurred level is never stored)
      fused_sweep_levels  levels whose anticausal-x and causal-y sweeps are one kernel (k_vv_xbyf: one R + one W)
      source_fused     level 0 is never materialised: k_src_index writes one 4-byte index plane; the causal x sweep and the
                       level-0 collapse read the frames (through that plane) instead of six level-0 planes
      implicit_mask    the level-0 mask plane is never read (a step function of x); the fused sweep still writes its blur
      coarse_from      > 0: levels coarse_from .. L-1 run in one launch (k_coarse): it reads G of level coarse_from, writes E of
                       that level and G, E of the levels above it; the per-level kernels are credited the finer levels only"""
    n = [w * h for w, h in zip(level_w, level_h)]
    L = len(n)
    P = n[0]
    inputs = (frame_px_a + frame_px_b) * 3 * bytes_per_sample
    s1 = inputs + 2 * P * 3 * 4
    s2 = sum(7 * 4 * (3 * n[l] + n[l + 1]) for l in range(L - 1))
    s3 = sum(4 * (10 * n[l] + 9 * n[l + 1]) for l in range(L - 1)) + 4 * 10 * n[L - 1]
    F = min(fused_sweep_levels, L - 1)
    m0 = 6 if implicit_mask else 7  # level-0 planes that exist as inputs of the blur
    x_fwd = x_fwd_src = x_bwd = y_fwd = y_bwd = xbyf = 0
    Lr = coarse_from if coarse_from > 0 else L - 1  # levels [0, Lr) are reduced / collapsed by per-level launches
    for l in range(Lr):
        rd = 4 * n[l] * (m0 if l == 0 else 7)
        wr = 4 * n[l] * 7
        if l == 0 and source_fused:
            x_fwd_src += inputs + 4 * P + 4 * n[0] * m0  # frames + index plane in, six (or seven) x-swept planes out
        else:
            x_fwd += rd + (4 * n[l] * m0 if l == 0 else wr)
        if l < F:
            xbyf += rd + wr
        else:
            x_bwd += rd + (4 * n[l] * m0 if l == 0 else wr)
            y_fwd += wr + wr
        y_bwd += wr + (7 * 4 * n[l + 1] if fused_decimate else wr)
    decimate = 0 if fused_decimate else sum(7 * 4 * (n[l] + n[l + 1]) for l in range(Lr))
    if L > 1:
        g0_in = (inputs + 4 * P) if source_fused else 4 * 6 * P
        collapse_l0 = g0_in + (0 if implicit_mask else 4 * P) + 4 * 9 * n[1] + 3 * P * bytes_per_sample
    else:
        collapse_l0 = 0
    per_kernel = {
        "compose": 4 * P if source_fused else s1,  # source-fused: the index plane
        "seam": 2 * bytes_per_sample * level_w[0],  # two mid rows
        "mask": 0 if implicit_mask else 4 * P,
        "vv_x_fwd": x_fwd, "vv_x_fwd_src": x_fwd_src, "vv_x_bwd": x_bwd, "vv_y_fwd": y_fwd, "vv_y_bwd": y_bwd, "vv_xbyf": xbyf,
        "decimate": decimate,
        "collapse_top": 0 if coarse_from > 0 else 4 * 10 * n[L - 1],
        "collapse": sum(4 * (10 * n[l] + 9 * n[l + 1]) for l in range(1, Lr)),
        "collapse_l0": collapse_l0,
        "coarse": 4 * 10 * sum(n[l] for l in range(coarse_from, L)) if coarse_from > 0 else 0,
    }
    return per_kernel, {"S1": s1, "S2": s2, "S3": s3, "total": s1 + s2 + s3}


def batches_of(n_pairs, rank, world, batch):
    """Config 4 as a schedule: this rank's contiguous shard of an n_pairs batch, cut into launch sequences of at most
    `batch` pairs -> list of (first, last+1) global pair indices."""
    lo, hi = shard_range(n_pairs, rank, world)
    return [(b, min(b + batch, hi)) for b in range(lo, hi, batch)]


def steps_per_sequence(n_local, batch, n_seqs_per_step, steps):
    """How many consecutive steps' shares a rank puts into ONE launch sequence: a shard smaller than a launch sequence (8 GPUs:
    4 pairs per rank and step, sequences of up to 16) is launched together with the shares of the following steps -- steps run
    back to back without host synchronisation anyway, every step keeps its own outputs and its own gather."""
    if n_seqs_per_step != 1 or n_local <= 0:
        return 1
    return max(1, min(batch // n_local, max(steps, 1)))


def sequence_sizes(count, per_seq, lanes):
    """`count` steps cut, in step order, into launch sequences of at most `per_seq` steps each; when there are more sequences than
    lanes their number is rounded up to a multiple of the lanes and the sizes are balanced, so that the lanes finish together
    instead of one sequence running on alone at the end (20 steps, 4 per sequence, 4 lanes: 3+3+3+3+2+2+2+2, not 4+4+4+4+4)."""
    if count <= 0:
        return []
    m = -(-count // per_seq)
    if per_seq > 1 and m > lanes and m % lanes:
        m = min(-(-m // lanes) * lanes, count)
    return [count // m + (1 if i < count % m else 0) for i in range(m)]


def exposure_match(proj_dst, proj_src, result, exposure, keep_black=True, stats_form=2, stats=None):
    """The reference's dead `transfer tran(X, T, X)` of ImageProcess.cpp:180-182, switched on: recolours the projected frame about
    to be warped, in place.  exposure 1: T is the projected frame it is stitched to; 2: T is the running mosaic; 0: nothing."""
    if exposure not in (0, 1, 2):
        raise ValueError(f"exposure {exposure!r} (0, 1 or 2)")
    if exposure:
        capi.dev_transfer(proj_dst, proj_src if exposure == 1 else result, out=proj_dst, stats=stats, stats_form=stats_form, keep_black=keep_black)
    return proj_dst


def exposure_stats_valid(m):
    """include/stitch_rig_exposure_temporal.h: a record the filter takes up -- twelve finite values, the six sds above 0."""
    m = np.asarray(m, np.float32)
    return bool(np.isfinite(m).all() and (m[[3, 4, 5, 9, 10, 11]] > 0).all())


def exposure_filter(m, keep, p):
    """The first-order filter of include/stitch_rig_exposure_temporal.h on ONE record, in float32 with every operation rounded:
    m the measured twelve statistics, p the state (12 floats) or None -> (used, state).  Not valid: (m, p).  Valid, no state:
    (m, m).  Valid, a state: u = m + (keep / 256) * (p - m), (u, u)."""
    m = np.asarray(m, np.float32).copy()
    if not exposure_stats_valid(m):
        return m, p
    if p is None:
        return m, m.copy()
    kf = np.float32(int(keep)) / np.float32(256)
    with np.errstate(all="ignore"):
        u = (m + (kf * (np.asarray(p, np.float32) - m).astype(np.float32)).astype(np.float32)).astype(np.float32)
    return u, u.copy()


def exposure_match_temporal(proj_dst, proj_src, result, exposure, keep_black, option, temporal, k):
    """exposure_match with the statistics it applies taken from `option` (stitch_chain's exposure_temporal) instead of measured:
    step k's record of fixed=, or the measured twelve filtered against temporal["state"][k].  Updates temporal in place."""
    import torch
    if option.get("fixed") is not None:
        u = np.asarray(option["fixed"][k], np.float32).reshape(12).copy()
    else:
        keep = int(option["keep"])
        if not 0 <= keep <= 255:
            raise ValueError(f"keep {keep} (0 .. 255)")
        s12 = torch.zeros(12, dtype=torch.float32, device=proj_dst.device)
        capi.dev_transfer(proj_dst, proj_src if exposure == 1 else result, out=torch.empty_like(proj_dst), stats=s12, stats_form=2, keep_black=keep_black)
        m = s12.cpu().numpy()
        p = temporal["state"][k]
        u, temporal["state"][k] = exposure_filter(m, keep, None if p is None else np.asarray(p, np.float32).reshape(12))
        temporal["measured"][k] = m
    temporal["used"][k] = u
    capi.dev_transfer_given_many([proj_dst], torch.from_numpy(u.reshape(1, 12)).to(proj_dst.device), out=[proj_dst], keep_black=keep_black)
    return proj_dst


def stitch_chain(frames, steps, opts=None, finish=True, num=19.0, den=20.0, plans=None, exposure=0, keep_black=True, seams=None, crop=None, formats=None,
                 residuals=None, seam_paths=None, exposure_temporal=None, scale=None):
    """The hot-path calls of ImageProcess::matching for a recorded stitch order, device resident.

    frames: list of (3,H,W) uint8 device tensors (unprojected).  steps: list of dicts with keys
    src (index of the frame to warp), p (8 doubles), offx, offy, ox, oy, cw, ch -- what the reference passes at
    ImageProcess.cpp:218-230; the first mosaic is projection(frames[start]).
    plans: optional dict kept by the caller across calls; the workspace of every canvas size met is created once and
    reused (a camera rig stitches every frame with the same geometry: without it half of a small panorama's time is
    the creation of the three workspaces).  Close them with close_plans(plans).
    exposure 1 / 2: every step first matches the frame's colours to the frame it is stitched to (the step's "mosaic_src") / to the
    running mosaic (exposure_match; include/stitch_exposure.h), keep_black leaving the projection's black corners black.
    seams: per step a capi.Seam or a tuple (sum_a_x, n_a, sum_ov_x, n_ov, ...) that replaces the step's seam scan
    (include/stitch_rig_seams.h): the single-set chain with given seams, the yardstick of a rig with fixed seams.
    crop: a pair ((x0, y0, w, h), mode) (include/stitch_rig_crop.h), applied with plain slicing: mode 1 the slice of the finished
    mosaic, mode 2 the finish pass on the slice of the unfinished one -- the single-set statement of a cropped rig.
    formats: (in_fmt, out_fmt, matrix) (include/stitch_rig_formats.h; the codes of include/stitch_rig_formats_yuv.h too), through the conversions on their own: the frames are
    capi.Images of in_fmt, unpacked first (capi.dev_unpack_many); the result is packed last (capi.dev_pack_many) and returned as a
    capi.Image of out_fmt at tight pitch.  A planar side stays a tensor -- the single-set statement of a rig with formats.
    residuals: dict(radius=r, domains=[one (ch, cw) uint8 device mask per step]) (include/stitch_rig_monitor.h): the chain also
    measures every step's record by capi.dev_pairs_residual on the exact inputs of its blend -- after the transfer, where exposure
    is set -- and returns (mosaic, records), records an (n_steps, words) int64 device tensor: the single-set statement of a rig
    with a monitor.  With residuals=None the return value and every byte stay as they are.
    seam_paths: dict(coverage=[(cov_a, cov_b) per step: (ch, cw) uint8 device masks], branches=[0 or 1 per step], max_step=2,
    margin=8, paths=None) (include/stitch_seam_path.h): every step finds its least-cost seam path by capi.dev_pairs_seam_path on
    the exact inputs of its blend -- after the transfer, where exposure is set -- and blends along it on a masked plan; with
    paths=[one int32 sequence of ch columns per step] nothing is found and the step blends along the given path.  The return value
    grows by `found`, a list of (path, cost) per step (an int32 device tensor; the cost is None for a given path): (mosaic, found),
    or (mosaic, records, found) with residuals -- the single-set statement of a rig with path seams.  With seam_paths=None the
    return value and every byte stay as they are.  With anchors=[per step an int32 sequence of ch columns, or None], weight= and
    cap= in the dict (include/stitch_seam_anchor.h) every step's finder takes the temporal term towards its anchor and `found`
    holds (path, cost, moved) per step; a caller that feeds a set's found paths into the next set's call as anchors states a rig
    that anchors per set.
    exposure_temporal: dict(keep=0 .. 255, state=None or [per step 12 floats or None]) or dict(fixed=[per step 12 floats])
    (include/stitch_rig_exposure_temporal.h), with exposure 1 or 2: the statistics a step's transfer applies are not the ones it
    measures.  keep/state: the step measures with capi.dev_transfer into a scratch output, filters the twelve statistics against
    the step's state by exposure_filter (numpy float32) and applies the result with capi.dev_transfer_given_many; fixed: the step
    applies the given record and measures nothing.  The return value grows by a last element, dict(state=[per step 12 floats or
    None], measured=[...], used=[...]) (measured None per step with fixed=): a caller that feeds a set's state into the next
    set's call states a rig that smooths.  With exposure_temporal=None the return value and every byte stay as they are.
    scale: (ow, oh) (include/stitch_rig_scale.h): the chain's planar output -- cropped and finished as above -- through
    capi.dev_scale_pack_many into out_fmt (planar without formats): the single-set statement of a rig with an output scale.  A planar
    result stays a tensor, now (3, oh, ow).  With scale=None the return value and every byte stay as they are.
    Returns the final uint8 mosaic tensor (after equalisation + luminance mix when finish=True, :237-268)."""
    if scale is not None:
        in_fmt, out_fmt, matrix = formats if formats is not None else (capi.PIX_PLANAR, capi.PIX_PLANAR, 0)
        result = stitch_chain(frames, steps, opts, finish, num, den, plans, exposure, keep_black, seams, crop,
                              None if formats is None else (in_fmt, capi.PIX_PLANAR, matrix), residuals, seam_paths, exposure_temporal)
        result, *extras = result if isinstance(result, tuple) else (result,)
        image = capi.dev_scale_pack_many([result], scale, out_fmt, matrix)[0]
        result = image.data if out_fmt == capi.PIX_PLANAR else image
        return (result, *extras) if extras else result
    if formats is not None:
        in_fmt, out_fmt, matrix = formats
        if in_fmt != capi.PIX_PLANAR:
            used_frames = {steps[0]["start"]} | {st["src"] for st in steps}  # the rig reads no other frame either
            frames = [capi.dev_unpack_many([f], matrix)[0] if i in used_frames else None for i, f in enumerate(frames)]
        result = stitch_chain(frames, steps, opts, finish, num, den, plans, exposure, keep_black, seams, crop, residuals=residuals, seam_paths=seam_paths,
                              exposure_temporal=exposure_temporal)
        result, *extras = result if isinstance(result, tuple) else (result,)
        result = result if out_fmt == capi.PIX_PLANAR else capi.dev_pack_many([result], out_fmt, matrix)[0]
        return (result, *extras) if extras else result
    proj = {}

    def projected(i):
        if i not in proj:
            proj[i] = capi.dev_project(frames[i])
        return proj[i]

    if seams is not None:
        seams = list(seams)
        if len(seams) != len(steps):
            raise ValueError("one seam per step")
    if residuals is not None and len(residuals["domains"]) != len(steps):
        raise ValueError("one residual domain per step")
    if seam_paths is not None:
        if seams is not None:
            raise ValueError("seam_paths and seams exclude each other")
        if len(seam_paths["coverage"]) != len(steps) or len(seam_paths["branches"]) != len(steps):
            raise ValueError("one pair of coverage masks and one branch per step")
        if seam_paths.get("paths") is not None and len(seam_paths["paths"]) != len(steps):
            raise ValueError("one path per step")
        if seam_paths.get("anchors") is not None and len(seam_paths["anchors"]) != len(steps):
            raise ValueError("one anchor (or None) per step")
    temporal = None
    if exposure_temporal is not None:
        if exposure not in (1, 2):
            raise ValueError("exposure_temporal needs exposure 1 or 2")
        fixed, state = exposure_temporal.get("fixed"), exposure_temporal.get("state")
        if (fixed is None) == ("keep" not in exposure_temporal):
            raise ValueError("exposure_temporal: either keep= (with state=) or fixed=")
        if len(fixed if fixed is not None else state if state is not None else steps) != len(steps):
            raise ValueError("one record (or None) per step")
        temporal = dict(state=list(state) if state is not None else [None] * len(steps), measured=[None] * len(steps), used=[None] * len(steps))
    result = projected(steps[0]["start"])
    used, records, found = [], [], []
    for k, st in enumerate(steps):
        key = (st["cw"], st["ch"]) if seam_paths is None else (st["cw"], st["ch"], "masked")
        plan = plans.get(key) if plans is not None else None
        if plan is None:
            plan = capi.Plan(st["cw"], st["ch"], opts, masked=seam_paths is not None)
            if plans is not None:
                plans[key] = plan
        elif plan in used:  # the same workspace twice in one chain: its seam record must be read before it is overwritten
            plan.status()
        if temporal is not None:
            exposure_match_temporal(projected(st["src"]), projected(st["mosaic_src"]) if exposure == 1 else None, result, exposure, keep_black, exposure_temporal,
                                    temporal, k)
        elif exposure:
            exposure_match(projected(st["src"]), projected(st["mosaic_src"]) if exposure == 1 else None, result, exposure, keep_black)
        if residuals is not None:
            records.append(capi.dev_pairs_residual([(projected(st["src"]), st["p"], st["offx"], st["offy"], result, st["ox"], st["oy"])], st["cw"], st["ch"],
                                                   [residuals["domains"][k]], residuals["radius"])[0])
        if seam_paths is not None:
            import torch
            inputs = (projected(st["src"]), st["p"], st["offx"], st["offy"], result, st["ox"], st["oy"])
            branch, tail = int(seam_paths["branches"][k]), ()
            if seam_paths.get("paths") is not None:
                given = seam_paths["paths"][k]
                path, cost = torch.as_tensor(given.cpu().numpy() if hasattr(given, "cpu") else given, dtype=torch.int32).to(result.device).contiguous(), None
            else:
                cov_a, cov_b = seam_paths["coverage"][k]
                extra = {}
                if seam_paths.get("anchors") is not None:
                    given = seam_paths["anchors"][k]
                    if given is not None:
                        given = torch.as_tensor(given.cpu().numpy() if hasattr(given, "cpu") else given, dtype=torch.int32).to(result.device).contiguous()
                    extra = dict(anchors=[given], weight=seam_paths["weight"], cap=seam_paths["cap"])
                paths, costs, *moved = capi.dev_pairs_seam_path([inputs], st["cw"], st["ch"], [cov_a], [cov_b], [branch], seam_paths.get("max_step", 2),
                                                                seam_paths.get("margin", 8), **extra)
                path, cost = paths[0], int(costs[0])
                tail = (int(moved[0][0]),) if moved else ()
            found.append((path, cost, *tail))
            out = torch.empty((3, st["ch"], st["cw"]), dtype=result.dtype, device=result.device)
            result = plan.pairs([inputs + (out,)], paths=[path], branches=[branch])[0]
        else:
            result = plan.pair(projected(st["src"]), st["p"], st["offx"], st["offy"], result, st["ox"], st["oy"], seam=None if seams is None else seams[k])
        used.append(plan)
    if crop is not None:
        (x0, y0, w, h), mode = crop
        if mode not in (1, 2):
            raise ValueError("crop mode 1 (after the finish pass) or 2 (before it)")
        if w < 1 or h < 1 or x0 < 0 or y0 < 0 or x0 + w > result.shape[2] or y0 + h > result.shape[1]:
            raise ValueError("the crop is empty or not inside the mosaic")
        if finish and mode == 1:
            capi.dev_finish(result, num, den)
        result = result[:, y0:y0 + h, x0:x0 + w].contiguous()
        if finish and mode == 2:
            capi.dev_finish(result, num, den)
    elif finish:
        capi.dev_finish(result, num, den)
    # the steps only depend on each other on the device; their seam scans are checked once, at the end (raises StitchError)
    try:
        for plan in used:
            plan.status()
    finally:
        if plans is None:
            for plan in used:
                plan.close()
    extras = (() if seam_paths is None else (found,)) + (() if temporal is None else (temporal,))
    if residuals is not None:
        import torch
        return (result, (torch.stack(records) if records else torch.empty((0, capi.residual_words(residuals["radius"])), dtype=torch.int64, device=result.device)),
                *extras)
    return (result, *extras) if extras else result


def close_plans(plans):
    for plan in plans.values():
        plan.close()
    plans.clear()


def levels_of(cw, ch, level_rule=0):
    length = min(cw, ch) if level_rule else max(cw, ch)
    return int(math.floor(math.log2(length)))


class MosaicGather:
    """Assembles a sharded batch on every rank: each rank contributes one block per step (`shape`: one finished uint8
    mosaic, or its whole shard of the step's batch, (n, 3, H, W)) and the step's blocks of all ranks are all-gathered (torch.distributed: backend "nccl" = RCCL over xGMI on the GPUs;
    "gloo" on CPU tensors in the tests).  The collective is asynchronous, so on the GPU it overlaps the next pair's
    kernels; a ring of `slots` input/output buffers bounds memory.  With keep=True every step's gathered block is
    retained (tests / small batches): result()[k, r] is the mosaic rank r produced at step k.

    Pairs are independent, so this end-of-pair exchange is the only communication of the batch configs."""

    def __init__(self, shape, device, world, rank, slots=2, keep=False, steps=0, group=None, force_collective=False, out_slots=None,
                 staged=False):
        import torch
        self.torch = torch
        self.world, self.rank, self.slots, self.keep, self.group = world, rank, slots, keep, group
        self.force_collective = force_collective  # issue the collective even with one rank (rehearsal of the N>1 path)
        # staged (bench.py's gloo rehearsal: several ranks drive ONE GPU, the collective runs on host tensors): submit() waits for
        # the block, moves it through host memory and returns with the gathered batch back on the device -- same buffers,
        # same step order, same slots as the RCCL form, only synchronous.
        self.staged = staged
        self.inp = [torch.empty(shape, dtype=torch.uint8, device=device) for _ in range(slots)]
        # input blocks are small (a rank's share of a step), gathered blocks are `world` times that: the input ring bounds how many
        # launch sequences may be in flight ahead of the exchange, the output ring only has to outlive one collective
        self.out_slots = (steps if keep else (out_slots or slots))
        self.out = [torch.empty((world,) + tuple(shape), dtype=torch.uint8, device=device) for _ in range(self.out_slots)]
        self.works = [None] * slots

    def input_slot(self, k):
        """Buffer to fill with step k's local mosaic(s); first waits for the gather that last used the slot.  May be
        called from several streams for the same step (each launch sequence of a step fills its own part of the block):
        every caller's stream waits, the handle is only replaced by submit()."""
        s = k % self.slots
        if self.works[s] is not None:
            self.works[s].wait()
        return self.inp[s]

    def gathered(self, k):
        """The gathered batch of step k, [rank][...] (valid until out_slots later steps have been submitted)."""
        return self.out[k if self.keep else k % self.out_slots]

    def submit(self, k):
        import torch.distributed as dist
        s = k % self.slots
        out = self.gathered(k)
        if self.world == 1 and not self.force_collective:
            out[0].copy_(self.inp[s])
            return
        if self.staged:
            torch = self.torch
            torch.cuda.current_stream(self.inp[s].device).synchronize()
            host_in = self.inp[s].cpu()
            host_out = torch.empty((self.world,) + tuple(host_in.shape), dtype=torch.uint8)
            dist.all_gather_into_tensor(host_out.flatten(0, 1), host_in, group=self.group)
            out.copy_(host_out)
            return
        # output viewed as the concatenation along dim 0 (the layout every backend accepts)
        self.works[s] = dist.all_gather_into_tensor(out.flatten(0, 1), self.inp[s], group=self.group, async_op=True)

    def drain(self):
        for i, wk in enumerate(self.works):
            if wk is not None:
                wk.wait()
                self.works[i] = None

    def result(self):
        assert self.keep
        return self.torch.stack(self.out)


def batch_order(n_pairs, world):
    """(step, rank) -> global pair index for a batch sharded with shard_range (contiguous per rank), or None
    where a rank has run out of pairs (ragged batches)."""
    table = {}
    for r in range(world):
        lo, hi = shard_range(n_pairs, r, world)
        for k in range(math.ceil(n_pairs / world)):
            table[(k, r)] = lo + k if lo + k < hi else None
    return table


class RankTransport:
    """What a band-split pair moves between ranks, over torch.distributed.  backend "nccl" (= RCCL over xGMI): device tensors
    go straight into send/recv/all_gather, ordered on the streams like any other kernel.  staged=True (gloo: the one-GPU
    test, where every rank drives the same device): tensors are staged through host memory."""

    def __init__(self, group=None, staged=False):
        import torch.distributed as dist
        self.dist, self.group, self.staged = dist, group, staged
        self.rank, self.world = dist.get_rank(group), dist.get_world_size(group)

    def send(self, t, dst):
        self.dist.send(t.cpu() if self.staged else t, dst, group=self.group)

    def recv(self, t, src):
        if self.staged:
            c = t.new_empty(t.shape, device="cpu")
            self.dist.recv(c, src, group=self.group)
            t.copy_(c)
        else:
            self.dist.recv(t, src, group=self.group)
        return t

    def all_gather(self, t):
        import torch
        out = torch.empty((self.world,) + tuple(t.shape), dtype=t.dtype, device="cpu" if self.staged else t.device)
        self.dist.all_gather_into_tensor(out.flatten(0, 1), t.cpu() if self.staged else t, group=self.group)
        return out.to(t.device) if self.staged else out

    def swap(self, to_prev, to_next, from_prev, from_next):
        """Neighbour exchange: to_prev goes to rank-1 (None on rank 0), to_next to rank+1 (None on the last rank); the
        neighbours' counterparts arrive in from_prev / from_next."""
        ops, keep = [], []
        P = self.dist.P2POp
        for t, peer, fn in ((to_prev, self.rank - 1, self.dist.isend), (to_next, self.rank + 1, self.dist.isend)):
            if t is not None:
                c = t.cpu() if self.staged else t
                keep.append(c)
                ops.append(P(fn, c, peer, group=self.group))
        stage = []
        for t, peer in ((from_prev, self.rank - 1), (from_next, self.rank + 1)):
            if t is not None:
                c = t.new_empty(t.shape, device="cpu") if self.staged else t
                stage.append((t, c))
                ops.append(P(self.dist.irecv, c, peer, group=self.group))
        if ops:
            for w in self.dist.batch_isend_irecv(ops):
                w.wait()
        if self.staged:
            for t, c in stage:
                t.copy_(c)


class LocalTransport:
    """RankTransport's interface for ranks that are THREADS of one process driving ONE device, each on its own HIP stream (the
    one-GPU form of the band split: tests, scripts/bench_band.py).  What crosses ranks never leaves the device and nobody waits
    on the host for the GPU: a hand-off is a device copy made on the sender's stream plus an event; the receiving thread takes
    the handle from a queue (a host-side hand-over of POINTERS, in enqueue order) and makes ITS stream wait for the event, so the
    bands' kernels are ordered on the device exactly as RCCL's stream-ordered send / recv orders them across GPUs."""

    def __init__(self, rank, world, queues):
        self.rank, self.world, self.qs = rank, world, queues

    @staticmethod
    def make_queues(world):
        import queue
        return {(a, b): queue.Queue() for a in range(world) for b in range(world) if a != b}

    def _post(self, t, dst):
        import torch
        c = t.clone()  # on this rank's stream: the source buffer may be rewritten by this rank's next launch
        ev = torch.cuda.Event()
        ev.record()
        self.qs[(self.rank, dst)].put((c, ev))

    def _take(self, src):
        import torch
        item = self.qs[(src, self.rank)].get()
        if item is None:
            raise RuntimeError(f"rank {src} failed")
        c, ev = item
        torch.cuda.current_stream().wait_event(ev)
        c.record_stream(torch.cuda.current_stream())  # allocated on the sender's stream, consumed on this one
        return c

    def send(self, t, dst):
        self._post(t, dst)

    def recv(self, t, src):
        t.copy_(self._take(src))
        return t

    def all_gather(self, t):
        import torch
        for d in range(self.world):
            if d != self.rank:
                self._post(t, d)
        return torch.stack([t if s_ == self.rank else self._take(s_) for s_ in range(self.world)])

    def swap(self, to_prev, to_next, from_prev, from_next):
        if to_prev is not None:
            self._post(to_prev, self.rank - 1)
        if to_next is not None:
            self._post(to_next, self.rank + 1)
        if from_prev is not None:
            from_prev.copy_(self._take(self.rank - 1))
        if from_next is not None:
            from_next.copy_(self._take(self.rank + 1))


PLANE_PIPELINE_MIN = None  # samples per plane of a band (rows x pitch) from which a level hands its state over plane by plane; None: never


class BandStitcher:
    """One pair split into row bands over the ranks of a node (BASELINE.json configs[4]; SURVEY.md 8(e)(ii): recurrence
    state hand-off, not a transpose).  Every rank holds the input frames and calls run() with the same arguments; it gets
    back ITS band of the mosaic, rows [rank*ch/world, (rank+1)*ch/world).  The per-band computation is capi.Band (HIP
    kernels); this class only sequences it and moves what crosses ranks through `transport`:
      * per split level, the causal y sweep waits for 3 doubles per column and plane from the rank above and passes its own
        on, then the anticausal sweep (+ decimation) the other way round;
      * the bands of the first replicated level are all-gathered and the coarse levels run on every rank;
      * before a split level is collapsed, two halo rows of G and E of the level above come from either neighbour."""

    def __init__(self, cw, ch, split_levels, transport, device, opts=None, fuse_sweeps=None, plane_pipeline_min=None, col_chunks=1):
        import torch
        self.t, self.dev = transport, device
        # the anticausal x sweep fused with the causal y sweep on the two finest levels (stitch_band_reduce_xy_fwd: one pass over a
        # level less).  The fused sweep finds its parallelism in the 64-row bands of a plane, and a rank's share of the rows has few
        # of them: at 24576 x 16384 one band gains, two lose and eight take twice as long (profiles/r03_config5_band.json).
        # Default: only when there is no split.
        self.fuse_sweeps = (transport.world == 1) if fuse_sweeps is None else bool(fuse_sweeps)
        self.rank, self.world = transport.rank, transport.world
        self.band = capi.Band(cw, ch, self.rank, self.world, split_levels, opts)
        self.Ls, self.geom = split_levels, self.band.geom
        f64 = dict(dtype=torch.float64, device=device)
        # recurrence states of all seven planes, [k][7][pitch] doubles per split level
        self.st_f = [torch.zeros(4 * 7 * g["pitch"], **f64) for g in self.geom[:-1]]  # causal state out (+ the band's last row)
        self.st_b = [torch.zeros(3 * 7 * g["pitch"], **f64) for g in self.geom[:-1]]  # anticausal state out
        self.res = [torch.zeros(3 * 7 * g["pitch"], **f64) for g in self.geom[:-1]]   # what a neighbour left
        # Optional (plane_pipeline_min = samples per plane of a band from which a level does it): the state crosses ranks PLANE BY
        # PLANE, so that rank r sweeps plane p while rank r+1 sweeps plane p-1 and the chain from rank to rank is 7 + N - 1
        # plane-steps long instead of 7 N.  Off by default: a one-plane launch has 192-384 wavefronts and streams at a quarter of
        # the seven-plane launch's rate, so on ONE GPU the split gets slower (24576 x 16384: 2 bands 31.4 -> 41.8 ms, 8 bands
        # 38.7 -> 41.6 from one host thread), and what it would gain across 8 GPUs (a 14-step chain of slower steps) is not
        # measurable on this pool.
        pmin = PLANE_PIPELINE_MIN if plane_pipeline_min is None else plane_pipeline_min
        self.per_plane = [pmin is not None and self.world > 1 and g["rows"] * g["pitch"] >= pmin for g in self.geom[:-1]]
        if self.per_plane[0]:
            self.band.set_level0(False)  # one plane at a time: level 0 must exist as planes
        # col_chunks = C > 1: the state crosses ranks in C column chunks (stitch_band_reduce_y_*_cols): columns are independent in a y
        # sweep, so rank r+1 starts on chunk c while rank r sweeps chunk c+1 and the chain of a level is N + C - 1 chunk-sweeps long
        # instead of N sweeps.  Levels with an odd width, the plane-by-plane form and the fused sweep keep one chunk.
        self.chunks = []
        for l, g in enumerate(self.geom[:-1]):
            C = 1 if (col_chunks <= 1 or g["w"] % 2 or self.per_plane[l] or (self.fuse_sweeps and l < 2)) else int(col_chunks)
            step = -(-g["pitch"] // (128 * C)) * 128  # columns per chunk: a multiple of 128
            self.chunks.append([(x0, min(x0 + step, g["pitch"])) for x0 in range(0, g["pitch"], step)] if C > 1 else None)
        pad = lambda n: -(-n // 128) * 128  # the chunk's state arrays have the launch's width: 128 columns per workgroup
        self.cst_f = [[torch.zeros(4 * 7 * pad(x1 - x0), **f64) for x0, x1 in ch_] if ch_ else None for ch_ in self.chunks]
        self.cst_b = [[torch.zeros(3 * 7 * pad(x1 - x0), **f64) for x0, x1 in ch_] if ch_ else None for ch_ in self.chunks]
        self.cres = [[torch.zeros(3 * 7 * pad(x1 - x0), **f64) for x0, x1 in ch_] if ch_ else None for ch_ in self.chunks]
        self.st_fp = [torch.zeros((7, 4 * g["pitch"]), **f64) if pp else None for pp, g in zip(self.per_plane, self.geom[:-1])]
        self.st_bp = [torch.zeros((7, 3 * g["pitch"]), **f64) if pp else None for pp, g in zip(self.per_plane, self.geom[:-1])]
        self.res_p = [torch.zeros((7, 3 * g["pitch"]), **f64) if pp else None for pp, g in zip(self.per_plane, self.geom[:-1])]

    def close(self):
        self.band.close()

    def run(self, frame, p, offx, offy, mosaic, ox, oy, out=None):
        """This rank's band of the mosaic.  Blocks only where the transport does (RCCL: nowhere on the host)."""
        gen = self.steps(frame, p, offx, offy, mosaic, ox, oy, out)
        T, val = self.t, None
        try:
            while True:
                req = gen.send(val)
                kind = req[0]
                val = (T.send(*req[1:]) if kind == "send" else T.recv(*req[1:]) if kind == "recv" else
                       T.all_gather(*req[1:]) if kind == "all_gather" else T.swap(*req[1:]))
        except StopIteration as e:
            out = e.value
        self.seam = self.band.status()
        return out

    def steps(self, frame, p, offx, offy, mosaic, ox, oy, out=None):
        """The band's launch sequence as a generator: it enqueues kernels and YIELDS what must cross ranks -- ("send", t, dst),
        ("recv", t, src) -> t, ("all_gather", t) -> stacked, ("swap", to_prev, to_next, from_prev, from_next) -- so that one host
        thread can interleave the sequences of several ranks (LocalBandGroup) and a rank of its own simply executes them (run)."""
        import torch
        B, r, N, Ls = self.band, self.rank, self.world, self.Ls
        g0 = self.geom[0]
        if out is None:
            out = torch.empty((3, g0["rows"], g0["w"]), dtype=frame.dtype, device=self.dev)
        B.compose(frame, p, offx, offy, mosaic, ox, oy)
        for l in range(Ls):
            n3 = 3 * 7 * self.geom[l]["pitch"]
            if self.per_plane[l]:
                n1 = 3 * self.geom[l]["pitch"]
                B.reduce_x(l)
                for pl in range(7):
                    res = (yield ("recv", self.res_p[l][pl], r - 1)) if r > 0 else None
                    B.reduce_y_fwd(l, pl, res, self.st_fp[l][pl])
                    if r < N - 1:
                        yield ("send", self.st_fp[l][pl][:n1], r + 1)
                for pl in range(7):
                    res = (yield ("recv", self.res_p[l][pl], r + 1)) if r < N - 1 else None
                    B.reduce_y_bwd(l, pl, self.st_fp[l][pl], res, self.st_bp[l][pl])
                    if r > 0:
                        yield ("send", self.st_bp[l][pl], r - 1)
                continue
            fuse = self.fuse_sweeps and l < 2  # as in a plan: the fused sweep on the two finest levels only (it loses on small levels)
            if self.chunks[l]:
                B.reduce_x(l)
                for c, (x0, x1) in enumerate(self.chunks[l]):  # causal sweep chunk by chunk, rank 0 first
                    res = (yield ("recv", self.cres[l][c], r - 1)) if r > 0 else None
                    B.reduce_y_fwd_cols(l, x0, x1, res, self.cst_f[l][c])
                    if r < N - 1:
                        yield ("send", self.cst_f[l][c][:self.cres[l][c].numel()], r + 1)
                for c, (x0, x1) in enumerate(self.chunks[l]):  # anticausal sweep + decimation chunk by chunk, last rank first
                    res = (yield ("recv", self.cres[l][c], r + 1)) if r < N - 1 else None
                    B.reduce_y_bwd_cols(l, x0, x1, self.cst_f[l][c], res, self.cst_b[l][c])
                    if r > 0:
                        yield ("send", self.cst_b[l][c], r - 1)
                continue
            if not fuse:
                B.reduce_x(l)
            # causal sweep, rank 0 first; then the anticausal sweep + decimation, last rank first.  A band's sweep is one chain
            # of dependent rows -- as long for seven planes as for one -- so all planes go in one launch and one message
            res = (yield ("recv", self.res[l], r - 1)) if r > 0 else None
            if fuse:
                B.reduce_xy_fwd(l, res, self.st_f[l])
            else:
                B.reduce_y_fwd(l, -1, res, self.st_f[l])
            if r < N - 1:
                yield ("send", self.st_f[l][:n3], r + 1)
            res = (yield ("recv", self.res[l], r + 1)) if r < N - 1 else None
            B.reduce_y_bwd(l, -1, self.st_f[l], res, self.st_b[l])
            if r > 0:
                yield ("send", self.st_b[l], r - 1)
        # the first replicated level: gather the bands, run the coarse levels on every rank
        gt = self.geom[Ls]
        mine = torch.empty((7, gt["rows"], gt["w"]), dtype=torch.float32, device=self.dev)
        B.rows(Ls, 2, 0, gt["rows"], mine, True)
        gathered = yield ("all_gather", mine)
        full = gathered.permute(1, 0, 2, 3).reshape(7, N * gt["rows"], gt["w"]).contiguous()
        B.top(full)
        for l in range(Ls - 1, -1, -1):
            if l + 1 < Ls and N > 1:  # halo rows of the level above: G (a, b) and E, from both neighbours (none without neighbours)
                gs = self.geom[l + 1]
                H, rows, w = gs["halo"], gs["rows"], gs["w"]
                for kind, planes in ((0, 6), (1, 3)):
                    mk = lambda: torch.empty((planes, H, w), dtype=torch.float32, device=self.dev)
                    first, last, above, below = mk(), mk(), mk(), mk()
                    B.rows(l + 1, kind, 0, H, first, True)
                    B.rows(l + 1, kind, rows - H, H, last, True)
                    yield ("swap", first if r > 0 else None, last if r < N - 1 else None, above if r > 0 else None, below if r < N - 1 else None)
                    if r > 0:
                        B.rows(l + 1, kind, -H, H, above, False)
                    if r < N - 1:
                        B.rows(l + 1, kind, rows, H, below, False)
            B.collapse(l, out if l == 0 else None)
        return out


class _Addr:
    """rank / world only: the BandStitchers of a LocalBandGroup never call a transport themselves."""

    def __init__(self, rank, world):
        self.rank, self.world = rank, world


class LocalBandGroup:
    """All N row bands of one pair on ONE device, driven by ONE host thread: every band has its own HIP stream, the bands'
    launch sequences (BandStitcher.steps) are advanced round-robin, and what crosses bands is a device copy on the sender's stream
    plus an event the receiver's stream waits for.  The host never waits for the GPU and never switches threads, so the device sees
    the pure dependency graph of the split -- the one-GPU rehearsal of what RCCL's stream-ordered send / recv gives across GPUs
    (8 bands at 24576 x 16384: 57 ms with host-staged hand-offs from 8 threads, 38.5 ms with device hand-offs from 8 threads,
    this class: see profiles/r03_config5_band.json)."""

    def __init__(self, cw, ch, split_levels, world, device, opts=None, fuse_sweeps=None, plane_pipeline_min=None, col_chunks=1):
        import collections
        import torch
        self.world, self.dev = world, device
        self.streams = [torch.cuda.Stream(device=device) for _ in range(world)]
        self.bands = [BandStitcher(cw, ch, split_levels, _Addr(r, world), device, opts, fuse_sweeps, plane_pipeline_min, col_chunks) for r in range(world)]
        self.box = collections.defaultdict(collections.deque)  # (src, dst) -> posted (tensor, event), FIFO

    def close(self):
        for b in self.bands:
            b.close()

    def _post(self, t, src, dst):
        import torch
        c = t.clone()
        ev = torch.cuda.Event()
        ev.record()
        self.box[(src, dst)].append((c, ev))

    def _take(self, src, dst):
        import torch
        if not self.box[(src, dst)]:
            return None
        c, ev = self.box[(src, dst)].popleft()
        torch.cuda.current_stream().wait_event(ev)
        c.record_stream(torch.cuda.current_stream())
        return c

    def _try(self, r, st):
        """Advance rank r's pending request as far as the posted messages allow; True when it is complete (st["val"] set)."""
        import torch
        req, N = st["req"], self.world
        kind = req[0]
        if kind == "send":
            self._post(req[1], r, req[2])
            st["val"] = None
            return True
        if kind == "recv":
            c = self._take(req[2], r)
            if c is None:
                return False
            req[1].copy_(c)
            st["val"] = req[1]
            return True
        if kind == "all_gather":
            if not st["posted"]:
                for d in range(N):
                    if d != r:
                        self._post(req[1], r, d)
                st["posted"], st["got"] = True, {r: req[1]}
            for s_ in range(N):
                if s_ not in st["got"]:
                    c = self._take(s_, r)
                    if c is None:
                        return False
                    st["got"][s_] = c
            st["val"] = torch.stack([st["got"][s_] for s_ in range(N)])
            return True
        _, to_prev, to_next, from_prev, from_next = req  # swap
        if not st["posted"]:
            if to_prev is not None:
                self._post(to_prev, r, r - 1)
            if to_next is not None:
                self._post(to_next, r, r + 1)
            st["posted"], st["got"] = True, {}
        for key, buf, src in (("p", from_prev, r - 1), ("n", from_next, r + 1)):
            if buf is not None and key not in st["got"]:
                c = self._take(src, r)
                if c is None:
                    return False
                buf.copy_(c)
                st["got"][key] = True
        st["val"] = None
        return True

    def run(self, frame, p, offx, offy, mosaic, ox, oy, outs=None):
        """-> the N bands of the mosaic (list, top to bottom)."""
        import torch
        N = self.world
        ready = torch.cuda.Event()
        ready.record()  # the inputs were produced on the caller's stream
        gens = [b.steps(frame, p, offx, offy, mosaic, ox, oy, None if outs is None else outs[r]) for r, b in enumerate(self.bands)]
        state = [{"req": None, "val": None, "posted": False, "got": None, "done": False, "out": None} for _ in range(N)]
        for s_ in self.streams:
            s_.wait_event(ready)
        left = N
        while left:
            progressed = False
            for r in range(N):
                st = state[r]
                if st["done"]:
                    continue
                with torch.cuda.stream(self.streams[r]):
                    while True:
                        if st["req"] is not None:
                            if not self._try(r, st):
                                break  # parked: the message has not been posted yet
                            st["req"] = None
                            progressed = True
                        try:
                            st["req"] = gens[r].send(st["val"])
                            st["val"], st["posted"], st["got"] = None, False, None
                        except StopIteration as e:
                            st["done"], st["out"] = True, e.value
                            left -= 1
                            progressed = True
                            break
            if not progressed:
                raise RuntimeError("band group: every rank waits for a message nobody has posted")
        done = torch.cuda.Event()
        for s_ in self.streams:  # the caller's stream continues behind every band
            done.record(s_)
            torch.cuda.current_stream().wait_event(done)
        for b in self.bands:
            b.seam = b.band.status()
        return [st["out"] for st in state]


# ---- descriptor matching: ImageProcess::matching's use of getImgPair (ImageProcess.cpp:117-137, :177-198) ------------------
MATCH_THRESHOLD = 20  # THRESHOLD, ImageProcess.h:18: frames i, j are neighbours when getImgPair(imgs[i], imgs[j]) has >= 20 pairs


def feature_order(descriptors, keypoints=None):
    """The order of Image::features, a std::map<std::vector<float>, VlSiftKeypoint> filled by siftAlgorithm
    (ImageProcess.cpp:44-99): descriptors sorted lexicographically as float vectors, an identical descriptor kept once -- the
    first inserted (std::map::insert keeps the existing entry).  `descriptors` (n, 128) in insertion order, `keypoints` any
    array with n rows (or None).  Returns (ordered descriptors, ordered keypoints or None, index into the inputs)."""
    import numpy as np
    d = np.ascontiguousarray(descriptors, dtype=np.float32)
    if d.ndim != 2 or d.shape[1] != capi.DESCRIPTOR_DIM:
        raise ValueError(f"expected (n, {capi.DESCRIPTOR_DIM}) descriptors, got {d.shape}")
    order = np.lexsort(d.T[::-1])  # stable: equal descriptors stay in insertion order
    s = d[order]
    keep = np.ones(len(order), bool)
    keep[1:] = np.any(s[1:] != s[:-1], axis=1)  # float ==, as the map's equivalence !(a < b) && !(b < a) (so -0 == +0)
    idx = order[keep]
    return d[idx], (np.asarray(keypoints)[idx] if keypoints is not None else None), idx


def _device_sets(desc_sets):
    import torch
    dev = torch.device("cuda", torch.cuda.current_device())
    return [torch.as_tensor(d, dtype=torch.float32).to(dev).contiguous().reshape(-1, capi.DESCRIPTOR_DIM) for d in desc_sets]


def match_counts(desc_sets, ratio=capi.RATIO_THRESHOLD):
    """N x N int matrix: [i][j] = the number of pairs getImgPair(imgs[i], imgs[j]) returns (data = frame i, queries = frame j;
    0 on the diagonal) for map-ordered descriptor sets, all ordered pairs in one batched launch sequence.  stichingMat[i][j]
    of matching() is `counts >= MATCH_THRESHOLD` (the reference skips the call for [i][j] once [j][i] is set, which only
    saves work: the flag is set either way)."""
    import numpy as np
    import torch
    sets = _device_sets(desc_sets)
    n = len(sets)
    ij = [(i, j) for i in range(n) for j in range(n) if i != j]
    outs = capi.dev_match_many([(sets[i], sets[j]) for i, j in ij], ratio, want_dist=False)
    counts = np.zeros((n, n), np.int64)
    if ij:
        got = torch.cat([o["count"] for o in outs]).cpu().numpy()
        for (i, j), c in zip(ij, got):
            counts[i, j] = int(c)
    return counts


def pair_lists(desc_src, kp_src, desc_dst, kp_dst, ratio=capi.RATIO_THRESHOLD):
    """The two point lists matching() hands to RANSAC for a stitched neighbour (ImageProcess.cpp:177-198): srcToDstPair =
    getImgPair(src, dst), dstToSrcPair = getImgPair(dst, src); the longer list wins (srcToDst on a strict >, else dstToSrc) and
    the other becomes its mirror.  Descriptors in map order, keypoints with the same rows (e.g. (n, 2) x/y).  Returns
    (src_to_dst, dst_to_src), each a pair of arrays (ImgPair.src keypoints, ImgPair.dst keypoints)."""
    import numpy as np
    kp_src, kp_dst = np.asarray(kp_src), np.asarray(kp_dst)
    a, b = _device_sets([desc_src, desc_dst])
    o_sd, o_ds = capi.dev_match_many([(a, b), (b, a)], ratio, want_dist=False)
    p_sd = o_sd["pairs"][: int(o_sd["count"].item())].cpu().numpy()
    p_ds = o_ds["pairs"][: int(o_ds["count"].item())].cpu().numpy()
    s2d = (kp_src[p_sd[:, 0]], kp_dst[p_sd[:, 1]])  # ImgPair(A = src keypoint[nn], B = dst keypoint[q])
    d2s = (kp_dst[p_ds[:, 0]], kp_src[p_ds[:, 1]])
    if len(p_sd) > len(p_ds):
        d2s = (s2d[1], s2d[0])
    else:
        s2d = (d2s[1], d2s[0])
    return s2d, d2s


# ---- map estimation and the whole of matching() from features (ImageProcess.cpp:101-268) -------------------------------------
def pair_maps(desc_src, kp_src, desc_dst, kp_dst, ratio=capi.RATIO_THRESHOLD, opts=None):
    """forward_H and backward_H of a stitched neighbour (ImageProcess.cpp:177-202) from map-ordered descriptors and (n, 2) x/y
    keypoints of the frame in the mosaic (src) and of the frame to warp (dst): both getImgPair calls, the longer-list rule and
    both RANSAC runs are enqueued back to back -- the rule is decided on the device from the two counts -- and the maps are read
    back once at the end.  Returns (p_fwd, p_bwd, info): 8 doubles each and the two info rows (forward, backward)."""
    import numpy as np
    import torch
    a, b = _device_sets([desc_src, desc_dst])
    dev = a.device
    ks = torch.as_tensor(np.ascontiguousarray(kp_src, dtype=np.float32)).to(dev).reshape(-1, 2)
    kd = torch.as_tensor(np.ascontiguousarray(kp_dst, dtype=np.float32)).to(dev).reshape(-1, 2)
    ns = ks.shape[0]
    x, y = torch.cat([ks[:, 0], kd[:, 0]]).contiguous(), torch.cat([ks[:, 1], kd[:, 1]]).contiguous()  # src rows, then dst rows
    o_sd, o_ds = capi.dev_match_many([(a, b), (b, a)], ratio, want_dist=False)
    cap = max(o_sd["pairs"].shape[0], o_ds["pairs"].shape[0])

    def padded(t):
        return torch.cat([t, t.new_zeros((cap - t.shape[0], 2))]) if t.shape[0] < cap else t
    sd, ds = padded(o_sd["pairs"]), padded(o_ds["pairs"])
    # srcToDstPair as (row of a src keypoint, row of a dst keypoint): getImgPair(src, dst) itself when it is the longer list
    # (strictly), else the mirror of getImgPair(dst, src) (:185-198); dstToSrcPair is its mirror either way
    use_sd = o_sd["count"] > o_ds["count"]
    s2d = torch.where(use_sd, torch.stack([sd[:, 0], sd[:, 1] + ns], 1), torch.stack([ds[:, 1], ds[:, 0] + ns], 1)).contiguous()
    count = torch.where(use_sd, o_sd["count"], o_ds["count"]).contiguous()
    lst = dict(src_x=x, src_y=y, dst_x=x, dst_y=y, pairs=s2d, count=count)
    p, info, _ = capi.dev_ransac_many([dict(lst, mirror=True), dict(lst, mirror=False)], opts, want_inliers=False)
    got = torch.cat([p, info.to(torch.float64)], 1).cpu().numpy()  # the one read-back
    return got[0, :8].copy(), got[1, :8].copy(), got[:, 8:].astype(np.int64)


def stitch_order(counts, threshold=MATCH_THRESHOLD):
    """The host logic of matching() (ImageProcess.cpp:101-175) and getMiddleIndex (:353-393) restated literally from the
    N x N matrix of getImgPair counts (match_counts): returns (start frame, [(srcIndex, dstIndex), ...]) -- dstIndex is warped
    onto the mosaic that already holds srcIndex."""
    n = len(counts)
    mat = [[False] * n for _ in range(n)]
    nxt = [[] for _ in range(n)]
    for i in range(n):
        for j in range(n):
            if i == j:
                continue
            if mat[j][i]:
                mat[i][j] = True
                nxt[i].append(j)
                continue
            if counts[i][j] >= threshold:
                mat[i][j] = True
                nxt[i].append(j)
    # getMiddleIndex: walk from an edge frame (exactly one neighbour; frame 0 without one) and take the middle of the walk
    edge = 0
    for i in range(n):
        if len(nxt[i]) == 1:
            edge = i
            break
    next_one = edge
    que = []
    for _index in range(n):
        if not que:
            que.append(edge)
        for i in range(n):
            if next_one == i:
                continue
            if mat[next_one][i]:
                if i < len(que):  # the reference compares the frame index i with the queue POSITIONS j = 0 .. size-1 (:377-382)
                    continue
                if i != edge:
                    que.append(i)
                next_one = i
                break
    start = que[len(que) // 2]
    order = []
    wait = [start]
    while wait:
        src = wait.pop(0)
        for dst in reversed(nxt[src]):
            if not mat[src][dst]:
                continue
            mat[src][dst] = mat[dst][src] = False
            wait.append(dst)
            order.append((src, dst))
    return start, order


class KeyPointTrack:
    """Every frame's key points through the steps of matching() (ImageProcess.cpp:226-227, :232), on the host: the warped frame's
    key points go through the forward map, then those of imgs[preStichingIndex] -- the frame warped by the step BEFORE (the start
    frame at the first step), whichever frame the step's srcIndex is -- move by the canvas offsets.  `kps` is a list of (n, 2)
    x/y arrays; `pre` is preStichingIndex."""

    def __init__(self, kps, start):
        import numpy as np
        self.kps = [np.array(k, dtype=np.float32).reshape(-1, 2) for k in kps]
        self.pre = start

    def stitched(self, src, dst, p_fwd, geom):
        """Step (srcIndex, dstIndex): frame `dst` has been warped onto the mosaic with the forward map p_fwd and the step geometry
        `geom` (capi.StepGeom).  `src` names the step; the reference moves imgs[preStichingIndex], not imgs[srcIndex]."""
        import numpy as np
        x, y, _, _ = capi.map_points(self.kps[dst][:, 0], self.kps[dst][:, 1], p_fwd, geom.min_x, geom.min_y)
        self.kps[dst] = np.stack([x, y], 1)
        x, y, _, _ = capi.shift_points(self.kps[self.pre][:, 0], self.kps[self.pre][:, 1], geom.ox, geom.oy)
        self.kps[self.pre] = np.stack([x, y], 1)
        self.pre = dst


def panorama_from_features(frames, features, opts=None, finish=True, num=19.0, den=20.0, return_steps=False, exposure=0, keep_black=True):
    """ImageProcess::matching (ImageProcess.cpp:101-268) from the frames and their SIFT features alone: frames is a list of
    (3, H, W) uint8 device tensors (unprojected), features a list of (descriptors (n, 128), keypoints (n, 2) x/y) in the
    std::map's order (feature_order).  Neighbour matrix, stitch order, per step both maps (pair_maps), the stitch step and the
    feature updates of :226-227.  exposure / keep_black: as stitch_chain; a step's dict then holds the transfer's twelve
    statistics ("exposure_stats") and a copy of the recoloured frame ("transferred").
    Returns the final mosaic (and, with return_steps, what every step used and produced)."""
    import numpy as np
    import torch
    desc = [np.ascontiguousarray(d, dtype=np.float32) for d, _ in features]
    start, order = stitch_order(match_counts(desc))
    track = KeyPointTrack([k for _, k in features], start)
    kps = track.kps  # updated in place by track.stitched
    proj = {}

    def projected(i):
        if i not in proj:
            proj[i] = capi.dev_project(frames[i])
        return proj[i]

    result = projected(start)
    steps = []
    for src, dst in order:
        p_fwd, p_bwd, info = pair_maps(desc[src], kps[src], desc[dst], kps[dst])
        if info[0][0] != capi.RANSAC_OK or info[1][0] != capi.RANSAC_OK:
            raise capi.StitchError(-1, f"frames {src} -> {dst}: no map (RANSAC status {int(info[0][0])} / {int(info[1][0])}, {int(info[0][1])} pairs)")
        extra = {}
        if exposure:
            stats = torch.zeros(12, dtype=torch.float32, device=result.device)
            exposure_match(projected(dst), projected(src), result, exposure, keep_black, stats=stats)
            if return_steps:
                extra = dict(exposure_stats=stats, transferred=projected(dst).clone())
        result, g, _seam = capi.dev_step(projected(dst), p_fwd, p_bwd, result, opts)
        track.stitched(src, dst, p_fwd, g)  # :226-227
        steps.append(dict(start=start, src=dst, mosaic_src=src, p=p_bwd, p_fwd=p_fwd, offx=g.min_x, offy=g.min_y, ox=g.ox, oy=g.oy, cw=g.cw, ch=g.ch,
                          out=result, info=info, **extra))
    if finish:
        result = result.clone() if return_steps and steps else result
        capi.dev_finish(result, num, den)
    return (result, steps) if return_steps else result


# ---- SIFT on the device: ImageProcess::ImageProcess (ImageProcess.cpp:12-25) and siftAlgorithm (:44-99) ----------------------
def sift_features(frames, opts=None, kp_cap=4096, feat_cap=None):
    """Projection -> gray -> SIFT for a list of (3, H, W) uint8 device tensors (unprojected), all frames in one launch sequence,
    then ONE read-back (counts, status, feature rows and their keypoints' x / y of every frame, packed) for the std::map's order
    (feature_order; the lexicographic order stays on the host).  Returns the list of (descriptors (n, 128), keypoints (n, 2)
    x/y) in map order that panorama_from_features takes."""
    import torch
    grays = [capi.dev_project_gray(f)[1] for f in frames]
    outs = capi.dev_sift_many(grays, opts, kp_cap, feat_cap)
    packed = []
    for o in outs:
        xy = o["kp"][:, 4:6].contiguous().view(torch.float32)[o["fkp"].long().clamp_(0, o["kp"].shape[0] - 1)]  # rows past the count are unused
        packed += [o["head"].view(torch.float32), o["desc"].reshape(-1), xy.reshape(-1)]
    host = torch.cat(packed).cpu().numpy() if packed else None  # waits for the stream
    feats, pos = [], 0
    for i, o in enumerate(outs):
        cap = o["desc"].shape[0]
        head = host[pos:pos + 6].view("int32")
        desc = host[pos + 6:pos + 6 + cap * capi.DESCRIPTOR_DIM].reshape(cap, capi.DESCRIPTOR_DIM)
        xy = host[pos + 6 + cap * capi.DESCRIPTOR_DIM:pos + 6 + cap * (capi.DESCRIPTOR_DIM + 2)].reshape(cap, 2)
        pos += 6 + cap * (capi.DESCRIPTOR_DIM + 2)
        if head[2] != capi.SIFT_OK:
            raise capi.StitchError(-1, f"frame {i}: SIFT capacities too small ({int(head[3])} keypoints, {int(head[4])} features found)")
        d, k, _ = feature_order(desc[:head[1]], xy[:head[1]])
        feats.append((d, k))
    return feats


def panorama_from_frames(frames, opts=None, finish=True, num=19.0, den=20.0, return_steps=False, sift_opts=None, kp_cap=4096,
                         feat_cap=None, exposure=0, keep_black=True):
    """The whole of ImageProcess::ImageProcess plus matching() from decoded frames alone: sift_features (kp_cap / feat_cap are
    its per-frame capacities; a frame that needs more raises StitchError with the counts found), then panorama_from_features."""
    return panorama_from_features(frames, sift_features(frames, sift_opts, kp_cap, feat_cap), opts, finish, num, den, return_steps, exposure, keep_black)


# ---- a rig calibrated from several captures (include/stitch_calibrate.h): the chain spelled out on the stage calls ---------------
CALIBRATE_MAX_PAIRS = 65536  # STITCH_CALIBRATE_MAX_PAIRS: the pairs of a list stitch_dev_ransac_many tests


def calibrate_from_features(frame_sizes, features, pooled_threshold=0, ransac_opts=None, ratio=capi.RATIO_THRESHOLD, match_threshold=MATCH_THRESHOLD):
    """matching() without the pixels, over several captures of the same cameras: frame_sizes = (width, height) per camera;
    features = per capture a list with, per camera, (descriptors (n, 128), keypoints (n, 2) x/y) in the std::map's order.
      * camera i's key points of all captures lie in one device array, capture k's rows from base[k][i] on;
      * getImgPair for every capture and ordered camera pair in one dev_match_many; pooled = the sum of the captures' counts;
      * the order is stitch_order(pooled, T), T = pooled_threshold or n_sets * match_threshold;
      * step (src, dst): the captures' accepted lists one behind the other, capture k's rows moved by base[k][src] and
        base[k][dst]; the longer-list rule once, on the pooled totals (the C chain decides it on the device; the counts are on the
        host here since the order needed them); both estimations on the pooled list, forward = the mirrored list first; the step's
        canvas; dst's points of all captures through the forward map, those of the camera warped before moved by the offsets.
    Returns a dict: start, steps (the keys of panorama_from_features's steps, "out" None), counts (n_sets, n, n), pooled (n, n),
    support (n_steps, n_sets, 2: per capture the pairs it put into the chosen list and its inliers of the forward map), width,
    height."""
    import numpy as np
    import torch
    n_sets, n = len(features), len(features[0])
    dev = torch.device("cuda", torch.cuda.current_device())
    desc = [_device_sets([d for d, _ in fs]) for fs in features]
    rows = np.array([[d.shape[0] for d in ds] for ds in desc], np.int64)
    base = np.concatenate([np.zeros((1, n), np.int64), np.cumsum(rows, 0)[:-1]])  # base[k][i]
    xy = [torch.as_tensor(np.concatenate([np.asarray(fs[i][1], np.float32).reshape(-1, 2) for fs in features])).to(dev) for i in range(n)]
    X, Y = [t[:, 0].contiguous() for t in xy], [t[:, 1].contiguous() for t in xy]
    kij = [(k, i, j) for k in range(n_sets) for i in range(n) for j in range(n) if i != j]
    outs = capi.dev_match_many([(desc[k][i], desc[k][j]) for k, i, j in kij], ratio, want_dist=False)
    lists = dict(zip(kij, outs))
    counts = np.zeros((n_sets, n, n), np.int32)
    if kij:
        for (k, i, j), c in zip(kij, torch.cat([o["count"] for o in outs]).cpu().numpy()):
            counts[k, i, j] = int(c)
    pooled = counts.sum(0, dtype=np.int32)
    start, order = stitch_order(pooled, pooled_threshold or n_sets * match_threshold)
    rw, rh = frame_sizes[start]
    steps, support, pre = [], [], start
    for src, dst in order:
        use_sd = int(pooled[src, dst]) > int(pooled[dst, src])
        parts = []
        for k in range(n_sets):
            shift = torch.tensor([int(base[k, src]), int(base[k, dst])], dtype=torch.int32, device=dev)
            if use_sd:  # (src row, dst row) as getImgPair(src, dst) lists them
                parts.append(lists[k, src, dst]["pairs"][:counts[k, src, dst]] + shift)
            else:       # the mirror of getImgPair(dst, src)
                parts.append(lists[k, dst, src]["pairs"][:counts[k, dst, src]].flip(1) + shift)
        off = np.concatenate([[0], np.cumsum([p.shape[0] for p in parts])])
        if off[-1] > CALIBRATE_MAX_PAIRS:
            raise capi.StitchError(-1, f"cameras {src} -> {dst}: the pooled list has {int(off[-1])} pairs (at most {CALIBRATE_MAX_PAIRS})")
        lst = dict(src_x=X[src], src_y=Y[src], dst_x=X[dst], dst_y=Y[dst], pairs=torch.cat(parts).contiguous())
        p, info, inl = capi.dev_ransac_many([dict(lst, mirror=True), dict(lst, mirror=False)], ransac_opts)
        got = torch.cat([p, info.to(torch.float64)], 1).cpu().numpy()
        p_fwd, p_bwd, info = got[0, :8].copy(), got[1, :8].copy(), got[:, 8:].astype(np.int64)
        if info[0][0] != capi.RANSAC_OK or info[1][0] != capi.RANSAC_OK:
            raise capi.StitchError(-1, f"cameras {src} -> {dst}: no map (RANSAC status {int(info[0][0])} / {int(info[1][0])}, {int(info[0][1])} pooled pairs)")
        win = inl[0][:int(info[0][3])].cpu().numpy()  # positions in the pooled list, increasing
        support.append([[int(off[k + 1] - off[k]), int(((win >= off[k]) & (win < off[k + 1])).sum())] for k in range(n_sets)])
        g = capi.step_geometry(frame_sizes[dst][0], frame_sizes[dst][1], p_fwd, rw, rh)
        capi.dev_map_points(X[dst], Y[dst], p_fwd, g.min_x, g.min_y, want_int=False)  # :226-227, every capture at once
        capi.dev_shift_points(X[pre], Y[pre], g.ox, g.oy, want_int=False)
        pre, rw, rh = dst, g.cw, g.ch
        steps.append(dict(start=start, src=dst, mosaic_src=src, p=p_bwd, p_fwd=p_fwd, offx=g.min_x, offy=g.min_y, ox=g.ox, oy=g.oy, cw=g.cw, ch=g.ch,
                          out=None, info=info))
    return dict(start=start, steps=steps, counts=counts, pooled=pooled, support=np.array(support, np.int32).reshape(len(steps), n_sets, 2), width=rw,
                height=rh)


def calibrate_from_sets(sets, pooled_threshold=0, sift_opts=None, ransac_opts=None, kp_cap=4096, feat_cap=None, ratio=capi.RATIO_THRESHOLD,
                        match_threshold=MATCH_THRESHOLD):
    """capi.dev_calibrate (stitch_dev_calibrate_u8) spelled out: sets is a list of captures, each a list of the n cameras'
    (3, H, W) uint8 device tensors (unprojected).  sift_features over the frames of ALL captures -- one dev_sift_many call, one
    read-back -- then calibrate_from_features."""
    n = len(sets[0])
    if any(len(fs) != n for fs in sets) or any(f.shape != g.shape for fs in sets for f, g in zip(fs, sets[0])):
        raise ValueError("every capture has the same cameras, each with one frame size")
    feats = sift_features([f for fs in sets for f in fs], sift_opts, kp_cap, feat_cap)
    return calibrate_from_features([(f.shape[2], f.shape[1]) for f in sets[0]], [feats[k * n:(k + 1) * n] for k in range(len(sets))], pooled_threshold,
                                   ransac_opts, ratio, match_threshold)


# ---- the same chain as ONE call of the C ABI (include/stitch_panorama.h): what a C++ caller gets ----------------------------------
panorama_c = capi.dev_panorama
calibrate_c = capi.dev_calibrate
