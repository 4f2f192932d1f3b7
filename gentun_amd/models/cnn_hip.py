"""HIP executor of the Genetic-CNN train step (MI355X path), population-batched.

One job trains ``Q`` groups at once, a group being one cross-validation fold
of one candidate architecture ("member"). Every candidate of a Genetic-CNN
search space shares the same *superset* network -- per stage an input conv,
``K`` DAG node convs, an output conv and a 2x2 pool -- and differs only in
which nodes exist and which node outputs each node sums
(gentun/models/keras_models.py:46-118). So instead of one launch per layer
per candidate, the job issues ONE launch per superset layer for all groups
that have it: activations live in slot tensors ``[Q][B][H][W][C]``, and a
per-launch group table (csrc/hip/cnn_conv.hip ``GroupRec``) tells each
group which slots to sum as input, where to write / accumulate its output
and where to apply a ReLU mask. Launch count per step is independent of the
population size and each launch is ``Q`` times larger -- the size at which
256 CUs fill (SURVEY.md §7.3 hard part 1).

Step (one HIP graph, replayed epochs x steps times):

  step_begin -> [cfg.augment: gt_augment writes the shifted / flipped batch] ->
  per stage: conv IN (first stage gathers the batch from the device-resident
  dataset, or reads the augmented batch), conv N_0..N_{K-1} (only groups whose node is
  active; fused N-ary Add of the node's predecessors), conv OUT (groups
  whose stage has a DAG), pool (per group: OUT or, without a DAG, IN) ->
  dense_fwd (+ReLU+dropout+partial logits) -> head (softmax + loss grad +
  dW2/db2/db1) -> dense_dgrad -> dense_wgrad_adam -> reverse: pool_bwd,
  per layer conv_wgrad (split-K partials) + dgrad (= conv_fwd with flipped
  weights, DAG gradient fan-out accumulation and ReLU masks fused per group)
  -> adam_segments (reduces the partials in fixed order).

Precision (``cfg.dtype``):

* ``fp32`` (default, the reference's TF/Keras float32): activations and
  gradients are fp32 tensors; every matrix product runs on the bf16 matrix
  cores as the exact 3-way split of its fp32 operands (six MFMA terms per
  product, error <= 2 fp32 ulps of each product before fp32 accumulation --
  csrc/hip/common.h, measured in tests/test_hip_fp32.py); the optimizer
  writes the three bf16 planes of every weight;
* ``bf16``: bf16 activations, one bf16 MFMA per product (fast mode).

Layouts: activations NHWC with channels padded to 8; fp32 master weights in
padded layouts whose padding is zero and stays zero; bf16 weight planes
(``[planes][...]``) written by the optimizer. Groups are member-major,
fold-minor.
"""

import math

import numpy as np
import torch

from ..ops import cnn_kernels as K
from ..utils import rng as _rng
from .cnn_engine import FoldJob
from .pop_schedule import PopulationSchedule

# conv weight-gradient streams of a job (the dense W1 optimizer gets one more): the wgrads of
# different layers are independent (own dz, own partial buffers), so they alternate over these
# streams and a small launch (few groups: 64 workgroups) does not serialise the backward tail behind
# one wgrad at a time (profiles/smallq_tiles_wgrad_streams_ab_r4.txt; 3 streams or a shared W1 stream
# were slower, stream_layout_ab_r4.txt). Module constants, not switches: tests vary them to check that
# results do not depend on the stream layout / issue path.
WGRAD_STREAMS = 2
# K4: fuse the 2x2 max-pool into the epilogue of the conv each group pools (and its backward into the
# producer of the pool's gradient) wherever a shape-specialised kernel runs the launch
POOL_FUSE = True
# eager training issues a whole epoch of steps from C++ (csrc/hip/step_prog.hip) in one host call;
# False: the Python issue path per step (what a captured step graph records)
NATIVE_STEPS = True

# True: fp32 3x3 layers with a Winograd F(2x2, 3x3) instantiation (csrc/hip/cnn_conv_wino.hip: the stage-2
# node / output convs of the S=(3,5) space) run their forward and data gradient on it, with the transformed
# weights re-derived from the fp32 masters after every optimizer step. 7-18 % faster than the direct kernel
# alone but 3.5 % slower in the population step, where its 256-VGPR / 68 KB workgroups share the CUs with
# the weight-gradient kernels (profiles/r6/wino_bench_r6.txt): off. Module constant, not a switch; tests
# flip it to check the executor path.
WINOGRAD = False

# layers (and directions) whose launches run the shape-specialised kernels read FRAGMENT-MAJOR weight planes
# (ConvArgs::wfrag: each MFMA A fragment one contiguous KB, 6-16 % per conv launch,
# profiles/r6/conv_wfrag_r6.txt), rewritten from the fp32 masters after every optimizer step; the optimizer
# then skips the row-major bf16 planes of those layers. Module constant; tests flip it.
WFRAG = True

# forward and data-gradient launches of the stage-2 3x3 fp32 shape (16x16, 56 -> 56 padded channels) ask for the
# 8-row tile with two-pass patch staging (ConvArgs::twopass: half the LDS per workgroup, 3 workgroups per CU
# instead of 2; bit-identical, profiles/r7/conv_s2_twopass_r7.txt) wherever the selection has it
# (gt_conv_fast_twopass). Module constant; tests flip it.
TWOPASS = True

# bytes of forward-only activation twins an evaluation may allocate for all groups of a job
EVAL_TWIN_BUDGET = 1 << 30


def pad8(c):
    return (c + 7) // 8 * 8


def round_up(x, m):
    return (x + m - 1) // m * m


def split_planes(w, npl):
    """``[npl][...]`` bf16 planes of an fp32 tensor: the exact split of
    csrc/hip/common.h (plane 0 = the RNE bf16 rounding; w = sum of planes)."""
    out = torch.empty((npl,) + tuple(w.shape), dtype=torch.bfloat16, device=w.device)
    r = w.float()
    for q in range(npl):
        out[q] = r.to(torch.bfloat16)
        r = r - out[q].float()
    return out


def fast_path_report(plan, dtype="fp32", ngroups=25, B=32, pad_images=True, batch_norm=False):
    """Which kernels a population step of this search space runs, probed without a GPU: the stored image
    size and per-stage channel padding the executor picks (cnn_kernels.padded_hw / stage_channel_pads),
    and per superset launch (every stage's input conv, node and output convs: forward, data gradient,
    weight gradient) whether a shape-specialised kernel runs it. ``generic_launches`` counts the
    launches of a superset step (all nodes present) left on the generic kernels."""
    prec = K.PREC[dtype]
    h0r, w0r, c0 = plan.input_shape
    kernels, nodes = list(plan.kernels_per_layer), list(plan.nodes)
    ks = [tuple(k) for k in plan.kernel_sizes]
    hw = K.padded_hw(h0r, w0r, len(kernels), batch_norm)
    h0, w0 = hw if pad_images else (h0r, w0r)
    pads = K.stage_channel_pads(c0, kernels, ks, h0, w0, prec, ngroups=ngroups, B=B)
    lib = K.lib()
    layers, generic, fast = [], 0, 0
    cin, cinr = pad8(c0), c0
    for s, (cp, k) in enumerate(zip(pads, ks)):
        H, W = h0 >> s, w0 >> s
        for kind, (KH, KW), ci, cir, n in (("in", k, cin, cinr, 1), ("node/out", (3, 3), cp, kernels[s], nodes[s] + 1)):
            first = s == 0 and kind == "in"
            f = K.layer_fast(KH, KW, ci, cp, H, W, prec, ngroups, B, cir, kernels[s], first)
            wino = bool(WINOGRAD and prec == 1 and (KH, KW) == (3, 3) and lib.gt_conv_wino_supported(ci, cp, H, W)
                        and lib.gt_conv_wino_supported(cp, ci, H, W))
            nl = n * (2 if first else 3)
            bad = n * sum(1 for x in (f if not first else f[::2]) if not x)
            generic += bad
            fast += nl - bad
            layers.append({"stage": s, "layer": kind, "k": KH, "hw": H, "cin_p": ci, "cout_p": cp,
                           "fwd_fast": f[0], "dgrad_fast": None if first else f[1], "wgrad_fast": f[2],
                           "winograd": wino})
        cin, cinr = cp, kernels[s]
    return {"stored_hw": [h0, w0], "stage_channels_padded": pads, "fast_launches": fast,
            "generic_launches": generic, "layers": layers}


class HipPopJob(FoldJob):

    def __init__(self, plan, x, y, folds, cfg, device, **kw):
        if cfg.dtype not in K.PREC:
            raise ValueError("HIP backend precision must be one of {}".format(sorted(K.PREC)))
        self.layout = "nhwc8f" if cfg.dtype == "fp32" else "nhwc8"
        if getattr(cfg, "dp_group", None) is not None and (
                kw.get("soft_targets") is not None or float(getattr(cfg, "label_smoothing", 0.0) or 0.0) > 0.0):
            raise ValueError("soft targets (label_smoothing / soft_targets) with dp_group are not supported by the "
                             "HIP executor (the torch executor supports it); train without data parallelism or "
                             "on the hard labels")
        # zero-padded storage of a slightly-smaller-than-power-of-two image (MNIST 28 x 28 -> 32 x 32):
        # every stage then runs the shape-specialised kernels (cnn_kernels.padded_hw)
        p0 = plan if plan is not None else kw["members"][0][0]
        h0r, w0r, _ = p0.input_shape
        hw = K.padded_hw(h0r, w0r, len(p0.kernels_per_layer), bool(getattr(cfg, "batch_norm", False)))
        self.pad_hw = hw if hw != (h0r, w0r) and getattr(cfg, "pad_images", True) else None
        super(HipPopJob, self).__init__(plan, x, y, folds, cfg, device, **kw)
        if self.device.type != "cuda":
            raise RuntimeError("the HIP backend needs a GPU device")
        self.L = K.lib()
        self.prec = K.PREC[cfg.dtype]
        self.npl = K.NPL[cfg.dtype]
        self.adt = torch.float32 if self.prec else torch.bfloat16      # activation / gradient storage
        self.bn = bool(getattr(cfg, "batch_norm", False))
        self._setup_dp()
        p0 = self.plan
        Q, B, dev = self.G, self.B, self.device
        self.Q = Q
        h0, w0, c0 = p0.input_shape
        if self.data.x.shape[-1] != pad8(c0):
            raise ValueError("dataset channels do not match the plan")
        self.classes = p0.classes
        if p0.classes > 16:
            raise ValueError("HIP head kernel supports at most 16 classes")
        if B > 64:
            raise ValueError("HIP head kernel supports batch_size <= 64")
        if max(p0.nodes) > K.MAXSLOT - 2:
            raise ValueError("at most {} nodes per stage".format(K.MAXSLOT - 2))
        self._build_topology()
        self._allocate()
        self.state = torch.zeros(8, dtype=torch.int32, device=dev)
        self.state_f = self.state.view(torch.float32)
        self.step_ctr = self.state[0:1]          # StepState.step_ctr (zeroed per epoch by the driver)
        self.eval_state = torch.zeros(8, dtype=torch.int32, device=dev)
        self.fold_ids_t = torch.tensor(self.fold_ids, dtype=torch.int32, device=dev)
        seeds = [_rng.stable_hash(self.member_seeds[self.gmember[q]], "dropout") & 0xFFFFFFFF for q in range(Q)]
        self.drop_seeds_t = torch.tensor(np.asarray(seeds, np.uint32).view(np.int32), device=dev)
        self._keep = []          # device group tables referenced by argument structs
        # side streams: every conv wgrad (alternating over WGRAD_STREAMS) and the dense W1 optimizer run
        # concurrently with the data-gradient chain (fork / join edges inside the captured step graph)
        ss = [torch.cuda.Stream(dev) for _ in range(WGRAD_STREAMS + 1)]
        self.wg_streams = ss[:WGRAD_STREAMS]
        self.side2 = ss[WGRAD_STREAMS]
        self.graph_streams = 2 + WGRAD_STREAMS     # capture stream + wgrad streams + W1 stream
        self._build_adam_table()
        self._build_args()

    # ------------------------------------------------------------ X5
    def _setup_dp(self):
        """Intra-candidate data parallelism on the HIP
        executor: ``cfg.dp_group`` ranks each train rows ``[r0, r1)`` of every
        group's batch -- the kernels see a batch of ``r1 - r0`` -- with the
        loss normalised by the FULL batch's real rows, dropout keyed by the
        full-batch row, and every gradient (conv weight gradients after their
        split-K reduce, dW1 written by the dense weight-gradient kernel in
        gradient-only mode, dW2 / db2 / db1) summed over the ranks by one
        all-reduce of a flat buffer before the identical optimizer step on
        every rank (RCCL over xGMI with the nccl backend; gloo through host
        memory). The step runs eagerly (no graph: the collective is host-side
        for gloo)."""
        grp = getattr(self.cfg, "dp_group", None)
        self.dp = None
        if grp is None:
            return
        if self.bn:
            raise ValueError("data parallelism with BatchNorm would need synchronised batch statistics")
        if self.aug is not None:
            raise ValueError("augment with dp_group is not supported by the HIP executor (the torch executor "
                             "supports it); train without data parallelism or without augmentation")
        import torch.distributed as dist
        world, rank = dist.get_world_size(grp), dist.get_rank(grp)
        B = self.B
        r0, r1 = rank * B // world, (rank + 1) * B // world
        if r1 <= r0:
            raise ValueError("data parallelism: batch {} over {} ranks leaves a rank without rows".format(B, world))
        self.dp = (grp, rank, world, r0, r1)
        self.capture_ok = False
        self.B_full = B
        self.epoch_idx_full = self.epoch_idx
        self.epoch_idx = torch.zeros((self.steps_per_epoch, self.G, r1 - r0), dtype=torch.int64, device=self.device)
        self.epoch_valid_full = self.epoch_valid
        self.epoch_valid = (self.epoch_valid_full - r0).clamp(0, r1 - r0).to(torch.int32).contiguous()
        self.B = r1 - r0

    def _new_epoch_order(self):
        if getattr(self, "dp", None) is None:
            return super(HipPopJob, self)._new_epoch_order()
        r0, r1 = self.dp[3], self.dp[4]
        local, self.epoch_idx, self.B = self.epoch_idx, self.epoch_idx_full, self.B_full
        try:
            super(HipPopJob, self)._new_epoch_order()        # the full batch order (same on every rank)
        finally:
            self.epoch_idx, self.B = local, r1 - r0
        self.epoch_idx.copy_(self.epoch_idx_full[:, :, r0:r1])

    def _dp_allreduce(self):
        """Sum every gradient over the data-parallel ranks (one flat buffer)."""
        import torch.distributed as dist
        grads = self._dp_grads
        flat = torch.cat([t.reshape(-1) for t in grads])
        if dist.get_backend(self.dp[0]) == "nccl":
            dist.all_reduce(flat, group=self.dp[0])
        else:                                           # gloo: through host memory
            host = flat.cpu()
            dist.all_reduce(host, group=self.dp[0])
            flat.copy_(host)
        o = 0
        for t in grads:
            n = t.numel()
            t.copy_(flat[o:o + n].view_as(t))
            o += n

    # ------------------------------------------------------------ topology
    def _build_topology(self):
        """Superset layers / per-group launch records (models/pop_schedule.py)
        plus the device geometry of every layer."""
        p0, Q = self.plan, self.Q
        h0r, w0r, _ = p0.input_shape
        h0, w0 = self.pad_hw or (h0r, w0r)
        self.sched = PopulationSchedule([self.members[self.gmember[q]][0] for q in range(Q)], hw=self.pad_hw)
        self.stages, self.layers = self.sched.stages, self.sched.layers
        # per-stage channel padding: every layer on the shape-specialised kernels where padding up allows
        ks = [tuple(k) for k in p0.kernel_sizes]
        self.stage_cp = K.stage_channel_pads(p0.input_shape[2], list(p0.kernels_per_layer), ks, h0, w0,
                                             self.prec, ngroups=Q, B=self.B)
        for L in self.layers:
            L.coutp = self.stage_cp[L.stage]
            L.cinp = pad8(L.cin) if L.kind == "in" and L.stage == 0 else \
                self.stage_cp[L.stage - 1] if L.kind == "in" else L.coutp
            L.Kdim = L.KH * L.KW * L.cinp
            L.TH = K.conv_tile_rows(L.H, L.W)
            band = K.wgrad_band(L.KH, L.KW, L.cinp, L.coutp, L.H, L.W, self.prec)
            L.pps, L.S = K.wgrad_split(self.B * L.H * L.W, L.Kdim, L.coutp, band=band)
            # split-K partials summed by a reduce launch right after the layer's wgrad, on the
            # weight-gradient stream (off the data-gradient chain); the optimizer then reads one gradient
            # (fused into the optimizer instead: 2-3 % slower, profiles/wgrad_reduce_fused_ab_r4.txt)
            L.wred = L.S > 1 and (L.coutp * L.Kdim) % 4 == 0
        self.last = self.sched.last
        hs, ws = h0 >> len(p0.kernels_per_layer), w0 >> len(p0.kernels_per_layer)
        if hs < 1 or ws < 1:
            raise ValueError("input too small for the pooling stages")
        self.final_hw = (hs, ws)
        self.final_hw_real = (h0r >> len(p0.kernels_per_layer), w0r >> len(p0.kernels_per_layer))
        self.final_cp = self.stage_cp[-1]

    # ------------------------------------------------------------ buffers
    def _allocate(self):
        Q, B, dev, p0 = self.Q, self.B, self.device, self.plan
        self.shapes = {}
        for st in self.stages:
            for L in st.layers:
                self.shapes[L.name] = (L.H, L.W, L.coutp)
            self.shapes[st.pool] = (st.H // 2, st.W // 2, self.stage_cp[st.s])
        self.act, self.grad = {}, {}
        for name, (hh, ww, cc) in self.shapes.items():
            self.act[name] = torch.zeros((Q, B, hh, ww, cc), dtype=self.adt, device=dev)
            self.grad[name] = torch.zeros((Q, B, hh, ww, cc), dtype=self.adt, device=dev)
        # layers where some group sums >1 input: the forward conv writes that
        # sum once ("<layer>_xin") and the layer's wgrad reads it as one slot
        for L in self.layers:
            if L.xin is not None:
                self.act[L.xin] = torch.zeros((Q, B, L.H, L.W, L.cinp), dtype=self.adt, device=dev)
        # BatchNorm: the conv writes its pre-activation z, the BN kernels write
        # relu(bn(z)) into the layer's activation slot
        self.zpre = {}
        if self.bn:
            for L in self.layers:
                self.zpre[L.name] = torch.zeros((Q, B, L.H, L.W, L.coutp), dtype=self.adt, device=dev)
                L.bn_chunk = K.bn_chunk_px(L.H, L.W, L.coutp)
                L.bn_nchunk = -(-(B * L.H * L.W) // L.bn_chunk)
                L.bn_stat = torch.zeros((Q, 2, L.coutp), dtype=torch.float32, device=dev)
                L.bn_run = torch.zeros((2, Q, L.coutp), dtype=torch.float32, device=dev)
                L.bn_part = torch.zeros((Q, L.bn_nchunk, 2, L.coutp), dtype=torch.float32, device=dev)
                L.g_gamma = torch.zeros((Q, L.coutp), dtype=torch.float32, device=dev)
                L.g_beta = torch.zeros((Q, L.coutp), dtype=torch.float32, device=dev)
        hs, ws = self.final_hw
        self.Fp = hs * ws * self.final_cp
        self.Up = round_up(p0.dense_units, 64)
        self.hdrop = torch.zeros((Q, B, self.Up), dtype=self.adt, device=dev)
        self.dH = torch.zeros((Q, B, self.Up), dtype=torch.float32, device=dev)
        # bf16 planes of dH written by head_bwd, read by the dense data gradient (no per-wave re-split)
        self.dHp = torch.zeros((self.npl, Q, B, self.Up), dtype=torch.int16, device=dev)
        self.dz_head = torch.zeros((Q, B, self.classes), dtype=torch.float32, device=dev)
        self.plog = torch.zeros((Q, self.Up // 16, B, self.classes), dtype=torch.float32, device=dev)
        segs = []
        for L in self.layers:
            segs.append(("w", L, (Q, L.coutp, L.KH, L.KW, L.cinp)))
            segs.append(("b", L, (Q, L.coutp)))
            if self.bn:
                segs.append(("gamma", L, (Q, L.coutp)))
                segs.append(("beta", L, (Q, L.coutp)))
        segs.append(("W1", None, (Q, self.Fp, self.Up)))
        segs.append(("b1", None, (Q, self.Up)))
        segs.append(("W2", None, (Q, self.Up, self.classes)))
        segs.append(("b2", None, (Q, self.classes)))
        total = sum(int(np.prod(s)) for _, _, s in segs)
        self.flat = torch.zeros(total, dtype=torch.float32, device=dev)
        self.m = torch.zeros_like(self.flat)
        self.v = torch.zeros_like(self.flat)
        off = 0
        self.views = {}
        for kind, L, shape in segs:
            n = int(np.prod(shape))
            view = (self.flat[off:off + n].view(shape), self.m[off:off + n].view(shape),
                    self.v[off:off + n].view(shape))
            if L is not None:
                setattr(L, kind, view)
            else:
                self.views[kind] = view
            off += n
        npl = self.npl
        wsegs = []
        for L in self.layers:
            L.w_bf = torch.zeros((npl, Q, L.coutp, L.KH, L.KW, L.cinp), dtype=torch.bfloat16, device=dev)
            L.wT_bf = torch.zeros((npl, Q, L.cinp, L.KH, L.KW, L.coutp), dtype=torch.bfloat16, device=dev)
            # Winograd layers: transformed weight planes of the forward and of the data gradient
            L.wino = bool(WINOGRAD and self.prec == 1 and (L.KH, L.KW) == (3, 3) and
                          self.L.gt_conv_wino_supported(L.cinp, L.coutp, L.H, L.W) and
                          self.L.gt_conv_wino_supported(L.coutp, L.cinp, L.H, L.W))
            if L.wino:
                R, Kc = K.wino_dims(L.cinp, L.coutp)
                L.wU = torch.zeros((3, Q, 16, R, Kc), dtype=torch.bfloat16, device=dev)
                R, Kc = K.wino_dims(L.coutp, L.cinp)
                L.wUT = torch.zeros((3, Q, 16, R, Kc), dtype=torch.bfloat16, device=dev)
                wsegs += [K.wino_segment(L.w[0], L.wU, False), K.wino_segment(L.w[0], L.wUT, True)]
            L.part_w = torch.zeros((L.S, Q, L.coutp, L.Kdim), dtype=torch.float32, device=dev)   # split-K partials
            L.part_b = torch.zeros((L.S, Q, L.coutp), dtype=torch.float32, device=dev)
        self.wino_tr = K.WinoTransform(wsegs, dev) if wsegs else None
        # fragment-major planes for every layer direction a shape-specialised kernel runs
        # (not with the fast path switched off, gt_conv_set_fast(0): the generic kernels refuse these planes)
        fspecs = []
        frag_on = WFRAG and K.fast_path_on(self.L)
        for L in self.layers:
            first = L.slots == ["input"]
            L.wfrag = L.wfragT = False
            if not frag_on or L.wino:
                continue
            nr = max(1, len(L.rows))
            if K._probe_conv(self.L, L.KH, L.KW, L.cinp, L.coutp, L.H, L.W, self.prec, nr, B, L.cout, True):
                _, nks = K.frag_order(L.KH, L.KW, L.cinp // 8, L.W, self.prec)
                L.wF = torch.zeros((npl, Q, -(-L.coutp // 16) * nks * 512), dtype=torch.bfloat16, device=dev)
                fspecs.append((L.w[0], L.wF, L.W, self.prec, False))
                L.wfrag = True
            if not first and K._probe_conv(self.L, L.KH, L.KW, L.coutp, L.cinp, L.H, L.W, self.prec, nr, B, L.cin,
                                           False):
                _, nks = K.frag_order(L.KH, L.KW, L.coutp // 8, L.W, self.prec)
                L.wTF = torch.zeros((npl, Q, -(-L.cinp // 16) * nks * 512), dtype=torch.bfloat16, device=dev)
                fspecs.append((L.w[0], L.wTF, L.W, self.prec, True))
                L.wfragT = True
            # the optimizer writes no row-major bf16 planes when nothing reads them
            L.bf_needed = not (L.wfrag and (L.wfragT or first))
        self.frag_tr = K.FragTransform(fspecs, dev) if fspecs else None
        self.gW2 = torch.zeros((Q, self.Up, self.classes), dtype=torch.float32, device=dev)
        self.gb2 = torch.zeros((Q, self.classes), dtype=torch.float32, device=dev)
        self.gb1 = torch.zeros((Q, self.Up), dtype=torch.float32, device=dev)

    def _gtab(self, rows):
        """Device GroupRec table from ``[(g, in_mask, out_flags)]``."""
        arr = np.zeros((max(1, len(rows)), 4), np.int32)
        for i, (g, im, of) in enumerate(rows):
            arr[i, 0], arr[i, 1], arr[i, 2] = g, im, of
        t = torch.from_numpy(arr).to(self.device)
        self._keep.append(t)
        return t

    # ------------------------------------------------------------ setup
    def _build_adam_table(self):
        segs, blocks = [], []

        def add(p, m, v, g, S, gstride, bf=None, bfT=None, tdims=None, pstrides=(0, 0)):
            sg = K.AdamSeg()
            sg.p, sg.m, sg.v, sg.g = p.data_ptr(), m.data_ptr(), v.data_ptr(), g.data_ptr()
            sg.bf = bf.data_ptr() if bf is not None else 0
            sg.bfT = bfT.data_ptr() if bfT is not None else 0
            sg.npl = self.npl
            sg.pstride_bf, sg.pstride_bfT = pstrides
            sg.n = p.numel()
            sg.gstride = gstride
            sg.S = S
            ntiles = 0
            if tdims is not None:
                sg.tG, sg.tCo, sg.tKH, sg.tKW, sg.tCi = tdims
                ntiles = K.adam_tiles(*tdims) if bfT is not None else 0
            sg.tiled = 1 if ntiles else 0
            idx = len(segs)
            segs.append(sg)
            if ntiles:
                blocks.extend((idx, t) for t in range(ntiles))
            else:
                for o in K.adam_blocks(p.numel()):
                    blocks.append((idx, o))

        # conv layers: one segment per (layer, group that has the layer)
        for L in self.layers:
            for q, _ in L.rows:
                p, m, v = (t[q] for t in L.w)
                S = 1 if L.wred else L.S            # reduced into split 0 by gt_wgrad_reduce
                if getattr(L, "bf_needed", True):
                    add(p, m, v, L.part_w[0, q], S, L.part_w[0].numel(), bf=L.w_bf[0, q], bfT=L.wT_bf[0, q],
                        tdims=(1, L.coutp, L.KH, L.KW, L.cinp), pstrides=(L.w_bf[0].numel(), L.wT_bf[0].numel()))
                else:                               # fragment-major planes: rewritten by gt_conv_wfrag
                    add(p, m, v, L.part_w[0, q], S, L.part_w[0].numel())
                p, m, v = (t[q] for t in L.b)
                add(p, m, v, L.part_b[0, q], S, L.part_b[0].numel())
                if self.bn:
                    for t, g in ((L.gamma, L.g_gamma), (L.beta, L.g_beta)):
                        p, m, v = (x[q] for x in t)
                        add(p, m, v, g[q], 1, g[q].numel())
        for name, g in (("b1", self.gb1), ("W2", self.gW2), ("b2", self.gb2)):
            p, m, v = self.views[name]
            add(p, m, v, g, 1, g.numel())
        arr = (K.AdamSeg * len(segs))(*segs)
        raw = bytes(memoryview(arr).cast("B"))
        self.adam_segs = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(self.device)
        self.adam_blocks = torch.tensor(np.asarray(blocks, np.int32).reshape(-1, 2), device=self.device)
        self.adam_nblocks = len(blocks)

    def _dense_sk_buffers(self, df, rows):
        """Range partials of a split-K dense forward at ``rows`` batch rows (training and evaluation
        launches get their own); a separate reduce launch sums them, so ``cnt`` (the arrival
        counters of the round-4 last-workgroup reduction) stays in the ABI, unused and 0."""
        nby, nut = -(-rows // 32), self.Up // 64
        part = torch.empty((self.Q * nby * nut * max(1, df.ks) * 4 * 2 * 64 * 4,), dtype=torch.float32,
                           device=self.device)
        self._keep.append(part)
        df.part, df.cnt = part.data_ptr(), 0

    def _conv_args(self, L, in_ptrs, out_ptrs, mask_ptrs, w, bias, relu, rows, gather=None, Cinp=None, Coutp=None):
        a = K.ConvArgs()
        for i, p in enumerate(in_ptrs):
            a.inp[i] = p
        for i, p in enumerate(out_ptrs):
            a.out[i] = p
        for i, p in enumerate(mask_ptrs):
            a.out_mask[i] = p
        a.relu = relu
        a.gather = gather or 0
        a.st = self.state.data_ptr()
        a.w = w.data_ptr()
        a.bias = bias.data_ptr() if bias is not None else 0
        a.gtab = self._gtab(rows).data_ptr()
        a.ngroups = len(rows)
        a.G, a.B, a.H, a.W = self.Q, self.B, L.H, L.W
        a.Cinp = L.cinp if Cinp is None else Cinp
        a.Coutp = L.coutp if Coutp is None else Coutp
        a.cout_real = L.cout if Coutp is None else L.cin      # data gradient: the layer's input channels
        a.KH, a.KW, a.TH = L.KH, L.KW, L.TH
        a.prec = self.prec
        a.wps = w[0].numel()                 # weights are [planes][...]
        return a

    def _set_twopass(self, a):
        """ConvArgs::twopass of a finished launch: 1 where the fast path is on and the selection has a
        two-pass staging kernel for these arguments."""
        a.twopass = 1 if TWOPASS and K.fast_path_on(self.L) else 0
        if a.twopass and self.L.gt_conv_fast_twopass(a) != 1:
            a.twopass = 0

    def _bn_args(self, L, train, pools=()):
        """``pools``: groups whose pool source is this layer (fused BN -> ReLU -> 2x2 max-pool)."""
        a = K.BnArgs()
        a.z, a.y = self.zpre[L.name].data_ptr(), self.act[L.name].data_ptr()
        a.gamma, a.beta = L.gamma[0].data_ptr(), L.beta[0].data_ptr()
        a.stat, a.run, a.part = L.bn_stat.data_ptr(), L.bn_run.data_ptr(), L.bn_part.data_ptr()
        a.ggamma, a.gbeta = L.g_gamma.data_ptr(), L.g_beta.data_ptr()
        a.gtab = self._gtab([(q, 0, (1 << 24) if q in pools else 0) for q, _ in L.rows]).data_ptr()
        a.W = L.W
        a.valid = self.epoch_valid.data_ptr()
        a.st = self.state.data_ptr()
        a.ngroups, a.G, a.B, a.HW, a.Cp = len(L.rows), self.Q, self.B, L.H * L.W, L.coutp
        a.nchunk, a.chunk_px = L.bn_nchunk, L.bn_chunk
        a.momentum, a.eps = self.cfg.bn_momentum, self.cfg.bn_eps
        a.train, a.prec = train, self.prec
        if self.pad_hw is not None:
            a.Hr, a.Wr = L.Hr, L.Wr          # statistics over the real pixels, zeros outside them
        return a

    def _stage_fwd_ops(self, st, gather_train, fuse):
        """Forward launches of one stage; ``fuse``: each group's pool source
        conv (with BatchNorm: its BN-apply launch) also writes the pooled
        output and the argmax mask."""
        src = self.sched.pool_source(st)
        x1 = self.sched.pool_x1(st)
        pool_of = {}
        if fuse:
            pool_of.setdefault(st.inp, set()).update(q for q in range(self.Q) if not src[q])
            pool_of.setdefault(x1, set()).update(q for q in range(self.Q) if src[q])
        ops = []
        for L in st.layers:
            first = L.slots == ["input"]
            out = self.zpre[L.name] if self.bn else self.act[L.name]
            pools = pool_of.get(L.name, set())
            cpools = set() if self.bn else pools
            a = self._conv_args(L, [self._slot_ptr(n) for n in L.slots], [out.data_ptr()], [],
                                L.wU if L.wino else L.wF if L.wfrag else L.w_bf, L.b[0], 0 if self.bn else 1,
                                [(q, im, 1 | ((1 << 24) if q in cpools else 0)) for q, im in L.rows],
                                gather=gather_train if first else None)
            a.wino = 1 if L.wino else 0
            a.wfrag = 1 if L.wfrag else 0
            if L.xin is not None:
                a.xsum = self.act[L.xin].data_ptr()
            if self.pad_hw is not None:
                a.Hr, a.Wr = L.Hr, L.Wr       # exact zeros outside the real image
            a.epi_bf16 = 1            # forward outputs never accumulate: bf16 output tile
            if cpools:
                a.pool_y, a.pool_mask = self.act[st.pool].data_ptr(), st.pmask.data_ptr()
            self._set_twopass(a)
            ops.append(("conv", a, L))
            if self.bn:
                b = self._bn_args(L, 1, pools)
                if pools:
                    b.pool_y, b.pool_mask = self.act[st.pool].data_ptr(), st.pmask.data_ptr()
                ops.append(("bn", b, L))
        return ops

    def _slot_ptr(self, name, grad=False):
        if name == "input":
            return self.data.x.data_ptr()
        t = (self.grad if grad else self.act).get(name)
        return t.data_ptr() if t is not None else 0       # a node no group has: never selected

    def _build_augment(self):
        """``cfg.augment``: the augmented batch, the gt_augment launch (csrc/hip/cnn_augment.hip) that
        fills it from the dataset every step, and the training copy of the forward launches whose first
        conv reads it. The conv and wgrad kernels keep their gather path (so the same shape-specialised
        kernels run): ``in[0]`` is the augmented batch and the table is the constant ``g * B + b``.
        ``self.fwd_ops`` stays the dataset-reading list the evaluation launches are copied from. Off
        (None): nothing is allocated and the training launches ARE ``self.fwd_ops``."""
        self.aug_args = self.aug_x = self.aug_table = None
        self.train_fwd_ops = self.fwd_ops
        if self.aug is None:
            return
        Q, B, dev = self.Q, self.B, self.device
        h0r, w0r, c0 = self.plan.input_shape
        hp, wp = self.pad_hw or (h0r, w0r)
        self.aug_x = torch.zeros((Q * B, hp, wp, pad8(c0)), dtype=self.adt, device=dev)
        self.aug_table = torch.arange(Q * B, dtype=torch.int64, device=dev).view(1, Q, B).repeat(
            self.steps_per_epoch, 1, 1).contiguous()
        a = K.AugArgs()
        a.src, a.out = self.data.x.data_ptr(), self.aug_x.data_ptr()
        a.gather, a.st = self.epoch_idx.data_ptr(), self.state.data_ptr()
        a.fold_ids, a.seeds = self.fold_ids_t.data_ptr(), self.drop_seeds_t.data_ptr()
        a.row_off = 0                     # data parallelism with augmentation is refused (_setup_dp)
        a.Q, a.B, a.Hp, a.Wp, a.Hr, a.Wr, a.Cp = Q, B, hp, wp, h0r, w0r, pad8(c0)
        a.shift, a.flip, a.prec = self.aug["shift"], 1 if self.aug["flip"] else 0, self.prec
        self.aug_args = a
        ops = []
        for kind, c, Lr in self.fwd_ops:
            if kind == "conv" and c.gather:
                c = K.ConvArgs.from_buffer_copy(c)
                c.inp[0], c.gather = self.aug_x.data_ptr(), self.aug_table.data_ptr()
            ops.append((kind, c, Lr))
        self.train_fwd_ops = ops

    def _build_args(self):
        """Pre-build every launch's argument struct (pointers are fixed)."""
        Q, B = self.Q, self.B
        gather_train = self.epoch_idx.data_ptr()
        self.fwd_ops = []
        # K4: the 2x2 max-pool (and its argmax mask) fused into the epilogue of
        # the conv each group pools (the stage's output conv, or its input conv
        # without a DAG) when that launch runs a shape-specialised kernel; the
        # separate pool kernel otherwise (and with BatchNorm, which normalises
        # after the conv)
        L_ = self.L
        fast_on = K.fast_path_on(L_)
        fuse_env = POOL_FUSE
        self.pool_fused = []
        for st in self.stages:
            hh, ww, cc = self.shapes[st.inp]
            # with BatchNorm the pool runs in the BN-apply launch (its chunks hold whole row pairs:
            # bn_chunk_px only halves 512 while the halves stay multiples of 2W)
            fuse_ok = fuse_env and (K.BN_CHUNK_PX % (2 * ww) == 0 and hh % 2 == 0 if self.bn else fast_on)
            sel = torch.tensor(self.sched.pool_source(st), dtype=torch.int32, device=self.device)
            self._keep.append(sel)
            st.sel = sel
            # argmax mask of the training forward (1 byte per pooled channel): pool_bwd reads it
            # instead of the 4 inputs of every cell
            st.pmask = torch.zeros((Q * B, hh // 2, ww // 2, cc), dtype=torch.uint8, device=self.device)
            ops = self._stage_fwd_ops(st, gather_train, fuse=fuse_ok)
            fused = fuse_ok and (self.bn or all(L_.gt_conv_fast_probe(a) > 0 for kind, a, _ in ops
                                                if kind == "conv" and a.pool_y))
            if not fused:
                ops = self._stage_fwd_ops(st, gather_train, fuse=False)
                x1 = self.act[self.sched.pool_x1(st)]
                ops.append(("pool", (self.act[st.inp].data_ptr(), x1.data_ptr(), sel.data_ptr(),
                                     self.act[st.pool].data_ptr(), Q * B, B, hh, ww, cc), st.pmask.data_ptr()))
            self.pool_fused.append(fused)
            self.fwd_ops.extend(ops)
        self._build_augment()
        prec = self.prec
        # ---- head
        df = K.DenseFwdArgs()
        df.x, df.wt, df.bias, df.out = (self.act[self.last].data_ptr(), 0, self.views["b1"][0].data_ptr(),
                                        self.hdrop.data_ptr())
        df.st, df.fold_ids, df.seeds = self.state.data_ptr(), self.fold_ids_t.data_ptr(), self.drop_seeds_t.data_ptr()
        df.G, df.B, df.Fp, df.Up = Q, B, self.Fp, self.Up
        df.drop_p, df.train, df.seed = self.cfg.dropout, 1, 0
        df.w2, df.plog, df.C = self.views["W2"][0].data_ptr(), self.plog.data_ptr(), self.classes
        df.prec, df.wps = prec, 0
        # split-K forward straight from the fp32 W1 master (csrc/hip/cnn_dense.hip dense_fwd_sk_kernel; Up is
        # a multiple of 64 by construction); the data gradient reads the master too: there is no W1 copy
        df.w1 = self.views["W1"][0].data_ptr()
        df.ks = int(self.L.gt_dense_fwd_splits(self.Fp))
        self._dense_sk_buffers(df, B)
        self.dense_fwd_args = df
        hd = K.HeadArgs()
        hd.h, hd.w2, hd.b2 = self.hdrop.data_ptr(), self.views["W2"][0].data_ptr(), self.views["b2"][0].data_ptr()
        hd.labels, hd.gather, hd.st = self.data.labels.data_ptr(), gather_train, self.state.data_ptr()
        hd.valid = self.epoch_valid.data_ptr()
        hd.dH, hd.gw2, hd.gb2, hd.gb1 = self.dH.data_ptr(), self.gW2.data_ptr(), self.gb2.data_ptr(), self.gb1.data_ptr()
        hd.eval_out = 0
        hd.dz = self.dz_head.data_ptr()
        hd.plog = self.plog.data_ptr()
        hd.G, hd.B, hd.Up, hd.C = Q, B, self.Up, self.classes
        hd.loss_ce = 1 if self.cfg.loss == "ce" else 0
        hd.drop_scale = 1.0 / (1.0 - self.cfg.dropout) if self.cfg.dropout < 1 else 0.0
        hd.eval = 0
        hd.prec = prec
        hd.dHp = self.dHp.data_ptr()
        self.head_args = hd
        # soft targets (cnn_engine.py "The target row"): the training step's head launch becomes gt_head_soft
        # over the same buffers; evaluation keeps gt_head on the hard labels. Off: nothing is built.
        self.head_soft_args = None
        if self.soft is not None or self.smooth_on_off is not None:
            hs = K.HeadSoftArgs()
            hs.head = hd                         # by value
            if self.soft is not None:
                hs.soft, hs.t_on, hs.t_off = self.soft.data_ptr(), 1.0, 0.0
            else:
                hs.soft, hs.t_on, hs.t_off = 0, float(self.smooth_on_off[0]), float(self.smooth_on_off[1])
            self.head_soft_args = hs
        dd = K.DenseDgradArgs()
        dd.dH, dd.wt, dd.dx = self.dH.data_ptr(), 0, self.grad[self.last].data_ptr()
        dd.dHp = self.dHp.data_ptr()
        dd.G, dd.B, dd.Fp, dd.Up = Q, B, self.Fp, self.Up
        dd.prec, dd.wps = prec, 0
        dd.w1 = self.views["W1"][0].data_ptr()      # the fp32 master (updated after dgrad)
        self.dense_dgrad_args = dd
        dw = K.DenseWgradAdamArgs()
        p, m, v = self.views["W1"]
        dw.x, dw.dH, dw.p, dw.m, dw.v = self.act[self.last].data_ptr(), self.dH.data_ptr(), p.data_ptr(), \
            m.data_ptr(), v.data_ptr()
        dw.wt, dw.st = 0, self.state.data_ptr()
        dw.G, dw.B, dw.Fp, dw.Up = Q, B, self.Fp, self.Up
        dw.Cp, dw.Cr, dw.Ur = self.final_cp, self.plan.kernels_per_layer[-1], self.plan.dense_units
        dw.prec, dw.wps = prec, 0
        self.dense_wgrad_args = dw
        if self.dp is not None:
            # X5: dW1 to a buffer (mode 1), all-reduced, then the update from it (mode 2)
            self.gW1 = torch.zeros((Q, self.Fp, self.Up), dtype=torch.float32, device=self.device)
            dw.gbuf, dw.mode = self.gW1.data_ptr(), 1
            self.dense_apply_args = K.DenseWgradAdamArgs.from_buffer_copy(dw)
            self.dense_apply_args.mode = 2
            df.row_off = self.dp[3]
            hd.valid_norm = self.epoch_valid_full.data_ptr()
            self._dp_grads = [t for L in self.layers for t in (L.part_w[0], L.part_b[0])] + \
                [self.gW1, self.gW2, self.gb2, self.gb1]
        # ---- backward (records: models/pop_schedule.py PopulationSchedule.backward)
        self.bwd_ops = []
        bn_done = set()
        # K4 backward: the gradient of a pool is un-pooled by its producer (the
        # dense data gradient for the last stage, the next stage's input-conv
        # data gradient otherwise) straight into the pool source's gradient
        fuse_bwd = fast_on and POOL_FUSE
        pool_stage = {st.pool: st for st in self.stages}
        self.unpool_fused = set()
        if fuse_bwd:
            st = self.stages[-1]
            hh, ww, cc = self.shapes[st.inp]
            dd.unpool_mask, dd.unpool_sel = st.pmask.data_ptr(), st.sel.data_ptr()
            dd.unpool_x0 = self.grad[st.inp].data_ptr()
            dd.unpool_x1 = self.grad[self.sched.pool_x1(st)].data_ptr()
            dd.Hs, dd.Ws, dd.Cp = hh, ww, cc
            self.unpool_fused.add(st.pool)
        for rec in self.sched.backward():
            if rec[0] == "pool_bwd":
                st = rec[1]
                if st.pool in self.unpool_fused:
                    continue
                hh, ww, cc = self.shapes[st.inp]
                x1 = self.sched.pool_x1(st)
                self.bwd_ops.append(("pool_bwd", (st.pmask.data_ptr(),
                                                  st.sel.data_ptr(), self.grad[st.pool].data_ptr(),
                                                  self.grad[st.inp].data_ptr(), self.grad[x1].data_ptr(),
                                                  Q * B, B, hh, ww, cc, 1, prec), None))
                continue
            kind, L, rows = rec
            first = L.slots == ["input"]
            if self.bn and L.name not in bn_done:
                # grad[L] is complete (every consumer's dgrad ran): BN backward
                # turns it into dz in place before the layer's wgrad / dgrad
                bn_done.add(L.name)
                ba = self._bn_args(L, 1)
                ba.y = self.grad[L.name].data_ptr()      # ReLU-masked grad in, dz out (in place)
                self.bwd_ops.append(("bn_bwd", ba, L))
            if kind == "wgrad":
                wa = K.WgradArgs()
                wslots = L.slots + ([L.xin] if L.xin is not None else [])
                for i, n in enumerate(wslots):
                    wa.inp[i] = self._slot_ptr(n)
                wa.gather = gather_train if first else 0
                if first and self.aug_args is not None:      # the augmented batch through its constant table
                    wa.inp[0], wa.gather = self.aug_x.data_ptr(), self.aug_table.data_ptr()
                wa.st = self.state.data_ptr()
                wa.dz = self.grad[L.name].data_ptr()
                wa.part_w, wa.part_b = L.part_w.data_ptr(), L.part_b.data_ptr()
                wa.gtab = self._gtab([(q, im, 0) for q, im in rows]).data_ptr()
                wa.ngroups = len(rows)
                wa.G, wa.B, wa.H, wa.W = Q, B, L.H, L.W
                wa.Cinp, wa.Coutp, wa.KH, wa.KW, wa.S, wa.pps = L.cinp, L.coutp, L.KH, L.KW, L.S, L.pps
                wa.prec = prec
                wa.cout_real = L.cout
                self.bwd_ops.append(("wgrad", wa, L))
            else:
                # dgrad = conv with flipped, transposed weights; per group the
                # fan-out flags (write / accumulate / ReLU mask per input slot)
                def dgrad_args(unpool):
                    a = self._conv_args(L, [self.grad[L.name].data_ptr()],
                                        [self._slot_ptr(n, grad=True) for n in L.slots],
                                        [self._slot_ptr(n) for n in L.slots],
                                        L.wUT if L.wino else L.wTF if L.wfragT else L.wT_bf,
                                        None, 0, [(q, 1, of | ((1 << 25) if unpool else 0)) for q, of in rows],
                                        Cinp=L.coutp, Coutp=L.cinp)
                    a.wino = 1 if L.wino else 0
                    a.wfrag = 1 if L.wfragT else 0
                    if unpool:
                        st = pool_stage[L.slots[0]]
                        a.pool_y, a.pool_mask = self.grad[st.inp].data_ptr(), st.pmask.data_ptr()
                        a.unpool_x1 = self.grad[self.sched.pool_x1(st)].data_ptr()
                        a.unpool_sel = st.sel.data_ptr()
                    self._set_twopass(a)
                    return a
                a = None
                if fuse_bwd and len(L.slots) == 1 and L.slots[0] in pool_stage:
                    a = dgrad_args(True)
                    if self.L.gt_conv_fast_probe_any(a):
                        self.unpool_fused.add(L.slots[0])
                    else:
                        a = None
                if a is None:
                    a = dgrad_args(False)
                self.bwd_ops.append(("conv", a, L))
        aa = K.AdamArgs()
        aa.segs, aa.blocks, aa.st = self.adam_segs.data_ptr(), self.adam_blocks.data_ptr(), self.state.data_ptr()
        self.adam_args = aa

    # -------------------------------------------------------------- protocol
    def _build_init_table(self):
        """Segment table of the one-launch Philox Glorot initialiser (K11):
        every conv kernel, W1 and W2 of every group; biases stay zero. Keys are
        (member seed, fold id, tensor name), so values do not depend on the
        batch composition."""
        Q = self.Q
        segs, blocks, seeds = [], [], []

        def add(t, d, r, fan_in, fan_out, name):
            assert t.is_contiguous() and t.numel() == Q * int(np.prod(d))
            seeds.append([_rng.stable_hash(self._fold_seed(g), name) & 0x7FFFFFFFFFFFFFFF for g in range(Q)])
            sg = K.InitSeg()
            sg.p = t.data_ptr()
            for i in range(4):
                sg.d[i], sg.r[i] = int(d[i]), int(r[i])
            sg.G = Q
            sg.tag = _rng.stable_hash("tag", name) & 0x7FFFFFFF
            sg.limit = math.sqrt(6.0 / (fan_in + fan_out))
            idx = len(segs)
            segs.append(sg)
            for o in range(0, t.numel(), 256):
                blocks.append((idx, o))

        for L in self.layers:
            add(L.w[0], (L.coutp, L.KH, L.KW, L.cinp), (L.cout, L.KH, L.KW, L.cin), L.cin * L.KH * L.KW,
                L.cout * L.KH * L.KW, L.name + ".w")
        hs, ws = self.final_hw
        hr, wr = self.final_hw_real          # W1 rows of padded pixels stay 0 (and get zero gradient)
        add(self.views["W1"][0], (hs, ws, self.final_cp, self.Up),
            (hr, wr, self.plan.kernels_per_layer[-1], self.plan.dense_units),
            self.plan.flatten, self.plan.dense_units, "dense1.w")
        w2 = self.views["W2"][0]
        add(w2, (1, 1, w2.shape[1], w2.shape[2]), (1, 1, self.plan.dense_units, self.plan.classes),
            self.plan.dense_units, self.plan.classes, "dense2.w")
        self.init_seeds = torch.tensor(np.asarray(seeds, np.int64), device=self.device)
        for k, sg in enumerate(segs):
            sg.seeds = self.init_seeds[k].data_ptr()
        arr = (K.InitSeg * len(segs))(*segs)
        self.init_segs = torch.frombuffer(bytearray(bytes(memoryview(arr).cast("B"))), dtype=torch.uint8
                                          ).to(self.device)
        self.init_blocks = torch.tensor(np.asarray(blocks, np.int32).reshape(-1, 2), device=self.device)
        ia = K.InitArgs()
        ia.segs, ia.blocks = self.init_segs.data_ptr(), self.init_blocks.data_ptr()
        self.init_args = ia
        self.init_nblocks = len(blocks)

    def init_params(self):
        """Glorot-uniform kernels (Philox, keyed by member, fold id and tensor
        name), zero biases -- Keras defaults, re-drawn per fold."""
        if getattr(self, "init_args", None) is None:
            self._build_init_table()
        self.flat.zero_()
        K.check(K.lib().gt_glorot_init(self.init_args, self.init_nblocks, self._stream()), "glorot_init")
        if self.bn:
            for L in self.layers:                # gamma 1 (padding channels stay 0), running stats (0, 1)
                L.gamma[0][:, :L.cout].fill_(1.0)
                L.bn_run[0].zero_()
                L.bn_run[1].fill_(1.0)
        self._refresh_copies()

    def _refresh_copies(self):
        """bf16 weight planes from the fp32 masters (the optimizer kernels
        keep them current afterwards)."""
        for L in self.layers:
            w = L.w[0]
            L.w_bf.copy_(split_planes(w, self.npl))
            L.wT_bf.copy_(split_planes(w.flip(2, 3).permute(0, 4, 2, 3, 1), self.npl))
        if self.frag_tr is not None:
            self.frag_tr.run(self._stream())
        if self.wino_tr is not None:
            self.wino_tr.run(self._stream())

    def reset_optimizer(self, lr):
        self.m.zero_()
        self.v.zero_()
        self.state_f[2:3].zero_()
        self.state_f[3:4].fill_(float(lr))
        self.state[6:7].fill_(1 if self.cfg.optimizer == "sgd" else 0)     # StepState.opt
        self.state_f[7:8].fill_(float(self.cfg.momentum))                  # StepState.momentum

    def snapshot(self):
        return (self.flat.clone(), self.m.clone(), self.v.clone(), self.state.clone(),
                [L.bn_run.clone() for L in self.layers] if self.bn else [])

    @property
    def can_rebind(self):
        # sequential folds on one job (SequentialFoldJob); the data-parallel
        # executor runs eagerly across ranks and is rebuilt per fold
        return self.dp is None

    def _rebind_device(self):
        # dropout keys read through this pointer by the captured step: in place
        self.fold_ids_t.copy_(torch.tensor(self.fold_ids, dtype=torch.int32))
        self.init_args = None            # Glorot seeds are keyed by fold id: rebuilt by init_params
        # a fresh job's step state: global_step keys the dropout masks of every step
        self.state.zero_()
        self.eval_state.zero_()

    def copy_biases_from(self, other):
        """Everything ``reset_weights`` keeps (keras_models.py:120-125 re-runs
        kernel initialisers only): conv / dense biases and, with BatchNorm,
        gamma / beta / running statistics of every group, from ``other`` (a job
        of the same members at the previous fold: SequentialFoldJob)."""
        mine = {L.name: L for L in self.layers}
        for L in other.layers:
            if L.name in mine:
                mine[L.name].b[0].copy_(L.b[0])
                if self.bn and other.bn:
                    mine[L.name].gamma[0].copy_(L.gamma[0])
                    mine[L.name].beta[0].copy_(L.beta[0])
                    mine[L.name].bn_run.copy_(L.bn_run)
        for name in ("b1", "b2"):
            self.views[name][0].copy_(other.views[name][0])

    def _kept_tensors(self):
        out = []
        for L in self.layers:
            out.append(L.b[0])
            if self.bn:
                out += [L.gamma[0], L.beta[0], L.bn_run]
        return out + [self.views["b1"][0], self.views["b2"][0]]

    def bias_state(self):
        return [t.clone() for t in self._kept_tensors()]

    def load_bias_state(self, state):
        for t, v in zip(self._kept_tensors(), state):
            t.copy_(v)
        self._refresh_copies()          # bf16 / split-plane copies of the parameters

    def restore(self, snap):
        self.flat.copy_(snap[0])
        self.m.copy_(snap[1])
        self.v.copy_(snap[2])
        self.state.copy_(snap[3])
        for L, r in zip(self.layers, snap[4]):
            L.bn_run.copy_(r)
        self._refresh_copies()

    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def _run_fwd(self, s, ops):
        L = self.L
        for kind, a, mk in ops:
            if kind == "conv":
                K.check(L.gt_conv_fwd(a, s), "conv_fwd")
            elif kind == "bn":
                K.check(L.gt_bn_fwd(a, s), "bn_fwd")
            elif mk is not None:
                K.check(L.gt_pool_fwd_mask(*a, mk, self.prec, s), "pool_fwd")
            else:
                K.check(L.gt_pool_fwd(*a, self.prec, s), "pool_fwd")

    def _fwd_plan(self, ops):
        plan = []
        for kind, a, mk in ops:
            if kind == "conv":
                plan.append(("k", "gt_conv_fwd", (a,), None, "conv_fwd"))
            elif kind == "bn":
                plan.append(("k", "gt_bn_fwd", (a,), None, "bn_fwd"))
            elif mk is not None:
                plan.append(("k", "gt_pool_fwd_mask", tuple(a) + (mk, self.prec), None, "pool_fwd"))
            else:
                plan.append(("k", "gt_pool_fwd", tuple(a) + (self.prec,), None, "pool_fwd"))
        return plan

    def _step_plan(self):
        """One training step up to the join of its streams, as launches
        ``("k", entry point, operands, stream, what)`` and event edges
        ``("rec" | "wait", stream, event id)``; stream ``None`` is the caller's
        (main) stream. Issued by :meth:`_exec_plan` (Python; also what a
        captured step graph records) or compiled once into a native
        :class:`~gentun_amd.ops.cnn_kernels.StepProgram`."""
        main = None
        plan = [("k", "gt_step_begin", (self.state.data_ptr(),), main, "step_begin")]
        if self.aug_args is not None:
            plan.append(("k", "gt_augment", (self.aug_args,), main, "augment"))
        plan += self._fwd_plan(self.train_fwd_ops)
        head = ("k", "gt_head", (self.head_args,), main, "head") if self.head_soft_args is None else \
            ("k", "gt_head_soft", (self.head_soft_args,), main, "head_soft")
        plan += [("k", "gt_dense_fwd", (self.dense_fwd_args,), main, "dense_fwd"), head,
                 ("k", "gt_dense_dgrad", (self.dense_dgrad_args,), main, "dense_dgrad")]   # reads W1 before its update
        side2 = self.side2
        nev = [0]

        def edge(src, dst):
            if src is not dst:
                plan.append(("rec", src, nev[0]))
                plan.append(("wait", dst, nev[0]))
                nev[0] += 1

        # W1 gradient + Adam only needs dH and the pooled features: it overlaps
        # the whole conv backward. Each layer's wgrad reads its final dz and its
        # (unchanged) inputs: it overlaps the layer's dgrad and everything after.
        # (Per-layer conv updates inside the backward, on the W1 stream, were 7-45 % slower:
        # profiles/adam_overlap_w1stream_ab_r4.txt; the last stage's update on its own: neutral,
        # adam_split_ab_r4.txt.)
        edge(main, side2)
        plan.append(("k", "gt_dense_wgrad_adam", (self.dense_wgrad_args,), side2, "dense_wgrad_adam"))
        wgs = self.wg_streams
        nwg = 0
        for kind, a, Lr in self.bwd_ops:
            if kind == "wgrad":
                ws = wgs[nwg % len(wgs)]
                nwg += 1
                edge(main, ws)
                plan.append(("k", "gt_conv_wgrad", (a,), ws, "conv_wgrad"))
                if Lr.wred:
                    plan.append(("k", "gt_wgrad_reduce", (a,), ws, "wgrad_reduce"))
            elif kind == "conv":
                plan.append(("k", "gt_conv_fwd", (a,), main, "conv_dgrad"))
            elif kind == "bn_bwd":
                plan.append(("k", "gt_bn_bwd", (a,), main, "bn_bwd"))
            else:
                plan.append(("k", "gt_pool_bwd_mask", tuple(a), main, "pool_bwd"))
        for stream in [side2] + list(wgs):
            edge(stream, main)
        return plan

    def _adam_plan(self):
        plan = [("k", "gt_adam_segments", (self.adam_args, self.adam_nblocks), None, "adam")]
        if self.frag_tr is not None:
            # the next step's convs read the fragment-major planes of the updated masters
            plan.append(("k", "gt_conv_wfrag", (K.C.addressof(self.frag_tr.args), self.frag_tr.nblocks), None,
                         "conv_wfrag"))
        if self.wino_tr is not None:
            # the next step's Winograd layers convolve with the transform of the updated masters
            plan.append(("k", "gt_wino_wtrans", (K.C.addressof(self.wino_tr.args), self.wino_tr.nblocks), None,
                         "wino_wtrans"))
        return plan

    def _exec_plan(self, plan):
        L = self.L
        main = torch.cuda.current_stream(self.device)
        evs = {}
        for op in plan:
            st = op[3] if op[0] == "k" else op[1]
            st = main if st is None else st
            if op[0] == "k":
                K.check(getattr(L, op[1])(*op[2], st.cuda_stream), op[4])
            elif op[0] == "rec":
                ev = torch.cuda.Event()
                ev.record(st)
                evs[op[2]] = ev
            else:
                st.wait_event(evs[op[2]])

    def train_step(self):
        self._exec_plan(self._step_plan())
        if self.dp is not None:
            self._dp_allreduce()
            K.check(self.L.gt_dense_wgrad_adam(self.dense_apply_args, self._stream()), "dense_wgrad_adam(apply)")
        self._exec_plan(self._adam_plan())

    def train_steps(self, n):
        """``n`` training steps issued eagerly: through the native step program
        (one host call; NATIVE_STEPS False or X5 data parallelism: the
        Python issue path per step)."""
        if self.dp is None and NATIVE_STEPS:
            prog = getattr(self, "_prog", None)
            if prog is None:
                prog = self._prog = K.StepProgram(self._step_plan() + self._adam_plan())
            prog.run(self._stream(), n)
            return
        for _ in range(n):
            self.train_step()

    def eval_batch(self):
        """Rows per evaluation launch (K13): ``cfg.eval_batch`` (default 256),
        capped at 256, at the validation fold size and by a 1 GB budget for
        the forward-only activation twins of ALL Q groups together (so a
        40-group job takes fewer rows per launch instead of 40x the memory);
        never below the training batch. Larger eval launches fill the GPU with
        Q groups x EB rows instead of Q x 32 (63 launches of 32 per
        2,000-sample fold become 8 of 256)."""
        per_img = sum(t[0, 0].numel() * t.element_size() for t in self.act.values())
        per_img += sum(t[0, 0].numel() * t.element_size() for t in self.zpre.values())
        per_img += self.Up * 4 * 2
        maxv = int(self.val_mat.shape[1])
        eb = min(int(getattr(self.cfg, "eval_batch", 256) or 256), 256, round_up(maxv, 32))
        eb = min(eb, max(1, int(EVAL_TWIN_BUDGET // max(1, per_img * self.Q))) // 32 * 32)
        return max(self.B, eb)

    def _eval_ops(self, EB):
        """Forward-only argument copies at batch EB on their own activation
        buffers (pointers of the training buffers remapped), the dense / head
        copies, and the buffers to keep alive. Built once per job and batch
        size: every fold's evaluation reuses the same twins."""
        cached = getattr(self, "_eval_cache", None)
        if cached is not None and cached[0] == EB:
            return cached[1]
        built = self._build_eval_ops(EB)
        self._eval_cache = (EB, built)
        return built

    def _build_eval_ops(self, EB):
        Q = self.Q
        remap, keep = {}, []

        def twin(t):
            e = torch.empty((Q, EB) + tuple(t.shape[2:]), dtype=t.dtype, device=t.device)
            remap[t.data_ptr()] = e.data_ptr()
            keep.append(e)
            return e
        for t in list(self.act.values()) + list(self.zpre.values()):
            twin(t)
        hdrop, plog = twin(self.hdrop), torch.empty((Q, self.Up // 16, EB, self.classes), dtype=torch.float32,
                                                    device=self.device)
        keep.append(plog)

        def rp(ptr):
            return remap.get(ptr, ptr)
        ops = []
        for kind, a, Lr in self.fwd_ops:
            if kind == "conv":
                b = K.ConvArgs.from_buffer_copy(a)
                for i in range(K.MAXSLOT):
                    b.inp[i], b.out[i] = rp(b.inp[i] or 0), rp(b.out[i] or 0)
                b.st = self.eval_state.data_ptr()
                b.xsum = 0
                b.pool_y = rp(b.pool_y or 0)
                b.pool_mask = 0                      # fused pool: output only
                b.B = EB
                self._set_twopass(b)                 # the evaluation batch may select another tile
                ops.append((kind, b, Lr))
            elif kind == "bn":
                b = K.BnArgs.from_buffer_copy(a)
                b.z, b.y, b.pool_y = rp(b.z or 0), rp(b.y or 0), rp(b.pool_y or 0)
                b.train = 0                          # running statistics
                b.pool_mask = 0
                b.B = EB
                b.nchunk = -(-(EB * b.HW) // b.chunk_px)
                ops.append((kind, b, Lr))
            else:
                xin, x1, sel, py, _qb, _b, hh, ww, cc = a
                ops.append((kind, (rp(xin), rp(x1), sel, rp(py), Q * EB, EB, hh, ww, cc), None))
        df = K.DenseFwdArgs.from_buffer_copy(self.dense_fwd_args)
        df.x, df.out, df.plog = rp(df.x), hdrop.data_ptr(), plog.data_ptr()
        df.B, df.train = EB, 0
        self._dense_sk_buffers(df, EB)
        hd = K.HeadArgs.from_buffer_copy(self.head_args)
        hd.h, hd.plog = hdrop.data_ptr(), plog.data_ptr()
        hd.B, hd.eval, hd.st = EB, 1, self.eval_state.data_ptr()
        return ops, df, hd, keep

    def evaluate(self):
        """Forward the validation folds in batches of ``eval_batch()`` rows
        (no dropout, running BatchNorm statistics); per-sample loss and
        accuracies summed over the real rows."""
        Q, dev = self.Q, self.device
        EB = self.eval_batch()
        maxv = self.val_mat.shape[1]
        nch = -(-maxv // EB)
        idx = torch.zeros((Q, nch * EB), dtype=torch.int64, device=dev)
        mask = torch.zeros((Q, nch * EB), dtype=torch.float32, device=dev)
        idx[:, :maxv] = self.val_mat
        mask[:, :maxv] = self.val_mask
        table = idx.view(Q, nch, EB).permute(1, 0, 2).contiguous()        # [nch][Q][EB]
        out = torch.zeros((nch, Q, EB, 3), dtype=torch.float32, device=dev)
        ops, df, hd, keep = self._eval_ops(EB)
        self._eval_keep = (table, out, keep)
        s = self._stream()
        L = self.L
        for c in range(nch):
            gptr = table[c].data_ptr()
            for kind, b, _ in ops:
                if kind == "conv" and b.gather:
                    b.gather = gptr
            self._run_fwd(s, ops)
            K.check(L.gt_dense_fwd(df, s), "dense_fwd(eval)")
            hd.gather, hd.eval_out = gptr, out[c].data_ptr()
            K.check(L.gt_head(hd, s), "head(eval)")
        res = out.permute(1, 0, 2, 3).reshape(Q, nch * EB, 3) * mask[:, :, None]
        sums = res.double().sum(1).float()      # fp64 accumulation: independent of the chunking
        return sums[:, 0], sums[:, 1], sums[:, 2]


# single-candidate name kept for callers of the fold-batched API
HipFoldJob = HipPopJob
