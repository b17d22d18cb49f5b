"""Batched self-play driver: the many-games-at-once counterpart of `CoachBPP.executeEpisode`
(xw_mcts/CoachBPP.py:50-99) that `CoachBPP.learn` and `bench.py` run.

Every engine slot plays one episode at a time.  The slots of a GPU are split into `groups` (default 2), each with its
own engine context, HIP stream and captured HIP graph of one simulation WAVE:

    rp_search_step      select / descend / terminal backups on device until each slot needs a leaf evaluated
    rp_leaf_stem        leaf states -> first convolution + max-pool of the CNN, computed from the packed state
                        (or rp_leaf_planes: FP32 NCHW planes for a generic evaluator)
    NNetWrapper.predict_from_stem   the rest of the CNN through PyTorch-ROCm (FP32)
    rp_commit_eval      mask / renormalise / expand / backup on device

With evaluator="rollout" the two middle steps are one kernel, rp_rollout_eval: every waiting leaf's value is the mean outcome of
`playouts` uniform random playouts and its prior is uniform -- plain MCTS with no network, the baseline a trained net is compared with.
playout_policy weighs a playout's legal moves by their item's size (rp_set_playout_policy); the default is uniform.
playout_landing weighs them by the row they land on as well (rp_set_playout_landing); the default, 0, is off.
rollout_prior replaces the uniform prior by one that weighs a legal move by its item's size and the row it lands on
(rp_set_rollout_prior); the default is uniform.

The groups' waves are launched alternately on their streams, so the latency-bound tree walk of one group runs while the
CNN of the other occupies the matrix cores.  Moves are played on device (`RP_MOVE_SAMPLE` / `RP_MOVE_ARGMAX_FIRST` / `_DRAW`) and a
finished slot immediately pulls the next instance of its group's pool, so the evaluator batch stays full until the pool
runs dry.
"""
import time

import numpy as np
import torch

from . import _lib


class _Group:
    def __init__(self, owner, index, games, seed):
        self.index = index
        self.G = games
        self.stream = torch.cuda.Stream(owner.device)
        follow = owner.move_rule == _lib.MOVE_INCUMBENT  # a new engine keeps no incumbents yet: the rule is set behind set_incumbent below
        self.eng = _lib.Engine(owner.W, owner.H, owner.N, games, int(owner.args.numMCTSSims), cpuct=float(owner.args.cpuct),
                               alpha=float(owner.args.alpha), move_rule=_lib.MOVE_ARGMAX_FIRST if follow else owner.move_rule, seed=seed,
                               tie_salt=(seed ^ 0x5DEECE66D) if owner.tie_salt is None else int(owner.tie_salt),
                               node_cap=owner.node_cap, edge_cap=owner.edge_cap, device=owner.device.index or 0,
                               stream=self.stream.cuda_stream, auto_restart=1, max_examples=owner.max_examples_per_group,
                               vis_cap=owner.vis_cap, reclaim=1 if owner.reclaim else 0)
        self.eng.set_step_cap(owner.step_cap)
        self.eng.set_compact_rows(owner.compact_rows)
        if owner.record_packings:
            self.eng.set_trace(True)
        if owner.record_best:
            self.eng.set_incumbent(True)
        if follow:
            self.eng.set_move_rule(_lib.MOVE_INCUMBENT)
        if owner.playout_incumbents:
            self.eng.set_incumbent_playouts(True)
        if owner.playout_policy != (0, 0):
            self.eng.set_playout_policy(*owner.playout_policy)
        if owner.playout_landing != 0:
            self.eng.set_playout_landing(owner.playout_landing)
        self.prior = owner.rollout_prior != (0, 0, 0)
        if self.prior:
            self.eng.set_rollout_prior(*owner.rollout_prior)
        self.use_stem = owner.use_stem
        self.host_evaluator = owner.host_evaluator
        self.wide_logits = owner.wide_logits
        self.rollout = owner.evaluator == "rollout"
        self.playouts = owner.playouts
        if self.rollout:  # no network: the uniform prior is written once, the playout kernel fills v every wave
            self.planes = None
            self.uniform_pi = torch.full((games, owner.A), float(np.float32(1) / np.float32(owner.A)), dtype=torch.float32, device=owner.device)
            # a rollout prior: the group's own rows, written by rollout_eval every wave
            self.prior_pi = torch.zeros((games, owner.A), dtype=torch.float32, device=owner.device) if self.prior else None
            self.rollout_v = torch.zeros(games, dtype=torch.float32, device=owner.device)
        elif self.use_stem:  # the engine computes the first conv + pool itself: no plane tensor at all
            self.channels_last = owner.channels_last
            self.resblock_kernel = owner.resblock_kernel
            fmt = torch.channels_last if self.channels_last else torch.contiguous_format
            self.stem = torch.zeros((games, 16, (owner.H + 1) // 2, (owner.W + 1) // 2), dtype=torch.float32, device=owner.device).contiguous(memory_format=fmt)
            # relu(stem) is only read by the library path of stage 0; k_resstage16 takes x alone and applies the ReLU itself, so with
            # the stage kernels the engine is handed NULL and writes 6.4 KB per leaf instead of 12.8 (half of k_leaf_stem's HBM bytes)
            self.fused = bool(owner.fuse_elementwise)
            stage0_kernel = owner.resblock_kernel and ((owner.H + 1) // 2) * ((owner.W + 1) // 2) <= 640  # BinPackingNNet.STAGE16_MAX_PIXELS
            self.stem_relu = torch.zeros_like(self.stem) if (owner.fuse_elementwise and not stage0_kernel) else None
            self.planes = None
        else:
            self.planes = torch.zeros((games, owner.N + 1, owner.H, owner.W), dtype=torch.float32, device=owner.device)
        self.graph = None
        self.pi = self.v = None
        self.raw_logits = False

    def refresh_weights(self, nnet):
        if self.use_stem:
            w, b = nnet.stem_params()
            self._stem_w, self._stem_b = w, b  # keep alive until the table kernel ran
            self.eng.stem_set_weights(w.data_ptr(), b.data_ptr())
            if self.fused and self.channels_last and self.resblock_kernel:
                self._frag_src = nnet.nnet.refresh_frags(self.eng)

    def leaf_inputs(self):
        """Evaluator input of the waiting leaves: the stem (first convolution + pool from the packed state) or the dense planes."""
        if self.use_stem:
            self.eng.leaf_stem(self.stem.data_ptr(), self.G, self.stem_relu.data_ptr() if self.stem_relu is not None else None, self.channels_last)
        else:
            self.eng.leaf_planes(self.planes.data_ptr(), self.G)

    def forward(self, nnet):
        """-> (policy rows, values).  With the fused evaluator the policy rows are the RAW logits and the softmax is taken inside the
        commit kernel: rp_commit_eval_logits up to LOGITS_MAX_ACTIONS, rp_commit_eval_logits_wide beyond (wide_logits; without it a
        wide board gets torch.softmax and rp_commit_eval)."""
        if self.use_stem:
            self.raw_logits = self.fused and (self.eng.A <= self.eng.LOGITS_MAX_ACTIONS
                                              or (self.wide_logits and self.eng.A <= self.eng.WIDE_LOGITS_MAX_ACTIONS))
            return nnet.predict_from_stem(self.stem, self.stem_relu, self.eng if self.fused else None, logits=self.raw_logits)
        self.raw_logits = False
        return nnet.predict_batch(self.planes)

    def commit(self, pi, v):
        if not self.raw_logits:
            commit = self.eng.commit_eval
        elif self.eng.A <= self.eng.LOGITS_MAX_ACTIONS:
            commit = self.eng.commit_eval_logits
        else:
            commit = self.eng.commit_eval_logits_wide
        commit(pi.data_ptr(), v.data_ptr())

    def wave_eager(self, nnet):
        if self.host_evaluator is not None:  # generic evaluator on the host: leaf states out, (pi, v) back (like nnet.predict, MCTS_bpp.py:87)
            n = self.eng.search_step()
            if n:
                rows, rem, slots = self.eng.leaf_states(n)
                pi, v = self.host_evaluator(rows, rem, slots)
                self.eng.commit_eval_host(pi, v)
            return
        self.eng.search_step(sync=False)
        if self.rollout:
            if self.prior:
                self.eng.rollout_eval(self.rollout_v.data_ptr(), self.G, self.playouts, pi_ptr=self.prior_pi.data_ptr())
                self.eng.commit_eval(self.prior_pi.data_ptr(), self.rollout_v.data_ptr())
                return
            self.eng.rollout_eval(self.rollout_v.data_ptr(), self.G, self.playouts)
            self.eng.commit_eval(self.uniform_pi.data_ptr(), self.rollout_v.data_ptr())
            return
        self.leaf_inputs()
        self.pi, self.v = self.forward(nnet)
        self.commit(self.pi, self.v)


class BatchedSelfPlay:
    def __init__(self, game, nnet, args, games, move_rule=_lib.MOVE_SAMPLE, seed=0, node_cap=0, edge_cap=0, max_examples=0,
                 use_graph=True, groups=2, step_cap=4, use_stem=True, fuse_elementwise=True, dense_small_convs=True, reclaim=True, vis_cap=0, compact_rows=True, channels_last=True, resblock_kernel=True, device=None,
                 tie_salt=None, host_evaluator=None, record_packings=False, wide_logits=True, evaluator="cnn", playouts=8, record_best=False,
                 playout_incumbents=False, playout_policy="uniform", rollout_prior="uniform", playout_landing=0):
        """evaluator: "cnn" (the network, the default) or "rollout": no network at all -- a leaf's value is the mean outcome of `playouts`
        uniform random playouts on the device (rp_rollout_eval) and its prior is uniform; nnet may then be None, the device is `device`
        or the current one, and the wave (search, playouts, commit) is captured into the HIP graph like the CNN wave.  Playouts are ranked
        against rewards_list like every terminal: with an empty list every outcome is +1 and the search learns nothing from them.
        wide_logits: action spaces beyond Engine.LOGITS_MAX_ACTIONS hand raw logits to rp_commit_eval_logits_wide (the softmax in the
        commit kernel, as on every smaller board); False keeps torch.softmax + rp_commit_eval for them (the A/B switch).
        record_packings: the engines record every move's placement (rp_set_trace); run() / run_from_seeds() return what they always
        return and the finished episodes' layouts are collected for pop_packings().
        record_best: the engines keep every episode's incumbent (rp_set_incumbent) -- the best complete packing its search tree saw,
        which the played one cannot beat; the finished episodes' incumbents are collected for pop_best_packings().  Tree terminals only,
        unless playout_incumbents is on.
        move_rule: a rule of _lib.  _lib.MOVE_INCUMBENT (the move follows the episode's incumbent where that is followable, else the first
        argmax of the visit counts: rp_engine.h) needs record_best=True, else ValueError.
        playout_incumbents: with record_best and evaluator="rollout", every playout is a candidate too (rp_set_incumbent_playouts): each
        evaluated leaf offers its best playout, and an incumbent's `tree_moves` / `playout` say where it came from.  ValueError
        without record_best or with another evaluator.
        playout_policy: with evaluator="rollout", how a playout chooses among the legal moves (rp_set_playout_policy): a name of
        _lib.PLAYOUT_POLICIES or a pair (w_pow, h_pow) -- a move of an item (w, h) weighs w^w_pow * h^h_pow.  "uniform" (the default)
        is (0, 0).  ValueError for anything else, and for a non-uniform policy with another evaluator.
        playout_landing: with evaluator="rollout", the landing power of the playouts (rp_set_playout_landing): 0 (the default), 1 or 2 --
        a legal move that lands on row t weighs (H - t)^playout_landing times its weight under playout_policy.  ValueError for anything
        else, and for a non-zero power with another evaluator.
        rollout_prior: with evaluator="rollout", the prior of a leaf (rp_set_rollout_prior): a name of _lib.ROLLOUT_PRIORS or a triple
        (w_pow, h_pow, land_pow) -- a legal move of an item (w, h) that lands on row t weighs w^w_pow * h^h_pow * (H - t)^land_pow.
        "uniform" (the default) is (0, 0, 0).  ValueError for anything else, and for a non-uniform prior with another evaluator.
        host_evaluator: optional callable (rows [n][H] uint64, remaining [n][N] uint8, slots [n]) -> (pi [n][A] float32, v [n]
        float32) that replaces the CNN -- any object with the reference's `predict` contract can sit behind it; the waves then run
        eagerly with one host round trip each.  tie_salt: salt of the deterministic `r == bl` tie (default: derived from seed)."""
        self.game, self.nnet, self.args = game, nnet, args
        self.W, self.H, self.N = game.bin_width, game.bin_height, game.num_items
        self.A = self.W * self.N
        if evaluator not in ("cnn", "rollout"):
            raise ValueError("evaluator must be 'cnn' or 'rollout', not %r" % (evaluator,))
        self.evaluator, self.playouts = evaluator, int(playouts)
        rollout = evaluator == "rollout"
        if rollout:
            if host_evaluator is not None:
                raise ValueError("evaluator='rollout' evaluates the leaves on the device: it cannot be combined with host_evaluator")
            if not 1 <= self.playouts <= _lib.Engine.MAX_PLAYOUTS:
                raise ValueError("playouts must be in 1..%d, not %d" % (_lib.Engine.MAX_PLAYOUTS, self.playouts))
            self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        else:
            if nnet.device.type != "cuda":
                raise RuntimeError("BatchedSelfPlay needs the evaluator on the GPU (args.cuda = True); there is no CPU path")
            self.device = nnet.device if device is None else device
        groups = max(1, min(int(groups), int(games)))
        self.G = int(games)
        self.move_rule, self.node_cap, self.edge_cap, self.step_cap = move_rule, node_cap, edge_cap, int(step_cap)
        self.reclaim, self.vis_cap = bool(reclaim), int(vis_cap)
        self.compact_rows = bool(compact_rows)  # evaluator rows = the waiting slots only, listed on the device (rp_set_compact_rows)
        self.max_examples_per_group = (int(max_examples) + groups - 1) // groups if max_examples else 0
        self.tie_salt, self.host_evaluator = tie_salt, host_evaluator
        self.wide_logits = bool(wide_logits)
        self.record_packings = bool(record_packings)  # set before the groups are built: their waves are captured with it
        self.record_best = bool(record_best)  # likewise
        if move_rule == _lib.MOVE_INCUMBENT and not self.record_best:
            raise ValueError("move_rule=MOVE_INCUMBENT follows the incumbents: it needs record_best=True")
        self.playout_incumbents = bool(playout_incumbents)  # likewise
        if self.playout_incumbents and not (self.record_best and rollout):
            raise ValueError("playout_incumbents needs record_best=True and evaluator='rollout'")
        self.playout_policy = _lib.playout_policy_powers(playout_policy)  # likewise
        if self.playout_policy != (0, 0) and not rollout:
            raise ValueError("a playout policy other than 'uniform' needs evaluator='rollout'")
        self.playout_landing = _lib.playout_landing_power(playout_landing)  # likewise
        if self.playout_landing != 0 and not rollout:
            raise ValueError("a playout landing power other than 0 needs evaluator='rollout'")
        self.rollout_prior = _lib.rollout_prior_powers(rollout_prior)  # likewise
        if self.rollout_prior != (0, 0, 0) and not rollout:
            raise ValueError("a rollout prior other than 'uniform' needs evaluator='rollout'")
        self._packings = []
        self._best = []
        self._pool_items = None
        self._pool_initial = None
        self.use_graph = bool(use_graph) and host_evaluator is None
        self.use_stem = bool(use_stem) and not rollout
        self.fuse_elementwise = bool(fuse_elementwise) and self.use_stem
        self.dense_small_convs = bool(dense_small_convs)
        self.channels_last = bool(channels_last) and self.fuse_elementwise
        self.resblock_kernel = bool(resblock_kernel) and self.channels_last
        if not rollout:
            nnet.nnet.use_resblock_kernel = self.resblock_kernel
        if self.channels_last:  # convolution weights in NHWC too, so MIOpen never converts per call
            nnet.nnet.to(memory_format=torch.channels_last)
        sizes = [self.G // groups + (1 if k < self.G % groups else 0) for k in range(groups)]
        # every group (and every rank) samples with the SAME seed: a move's draw depends on (seed, global episode id, move) only,
        # so episodes do not depend on how many groups or ranks share the pool
        self.groups = [_Group(self, k, sizes[k], int(seed) & 0x7FFFFFFFFFFFFFFF) for k in range(groups)]
        self.steps = 0
        self.first_id = 0

    @property
    def eng(self):
        """First group's engine (single-group callers, tests)."""
        return self.groups[0].eng

    def close(self):
        for g in self.groups:
            g.graph = None
            g.pi = g.v = g.stem = g.stem_relu = g.planes = g.uniform_pi = g.prior_pi = g.rollout_v = None
            g.eng.close()

    @property
    def device_bytes(self):
        return sum(g.eng.device_bytes for g in self.groups)

    # ---- waves -----------------------------------------------------------------------------------
    def prepare(self):
        """Warms the evaluator up (MIOpen picks its kernels on the first calls) and captures every group's wave -- the
        engine's kernels and the CNN's -- into one HIP graph each, so a wave costs one graph launch instead of ~40 kernel
        launches."""
        if self.host_evaluator is not None:
            return
        if self.fuse_elementwise and self.dense_small_convs:
            self.nnet.refresh_fused()
        if not self.use_graph:
            return
        for g in self.groups:
            if g.graph is not None:
                continue
            torch.cuda.synchronize(self.device)
            if self.evaluator == "cnn":
                with torch.cuda.stream(g.stream):
                    g.refresh_weights(self.nnet)
                    for _ in range(3):
                        g.forward(self.nnet)
                torch.cuda.synchronize(self.device)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=g.stream):
                g.wave_eager(self.nnet)
            torch.cuda.synchronize(self.device)
            g.graph = graph

    def invalidate_graph(self):
        """Call after the evaluator's weights were REPLACED (not updated in place), or after set_move_rule / set_sims:
        kernel arguments are baked into the captured graphs."""
        for g in self.groups:
            g.graph = None

    def step_group(self, g):
        with torch.cuda.stream(g.stream):
            if self.use_graph:
                if g.graph is None:
                    self.prepare()
                g.graph.replay()
            else:
                g.wave_eager(self.nnet)

    def step(self):
        """One simulation wave for every group (each on its own stream)."""
        for g in self.groups:
            self.step_group(g)
        self.steps += 1

    def set_move_rule(self, move_rule, onehot_examples=False):
        """Switches the move rule of every group; re-captures the waves.  _lib.MOVE_INCUMBENT needs record_best on (ValueError)."""
        if move_rule == _lib.MOVE_INCUMBENT and not self.record_best:
            raise ValueError("move_rule=MOVE_INCUMBENT follows the incumbents: set_record_best(True) first")
        for g in self.groups:
            g.eng.set_move_rule(move_rule, onehot_examples)
        self.move_rule = move_rule
        self.invalidate_graph()

    def set_record_packings(self, on=True):
        """Switches the placement trace of every group between pools (refused while episodes are being played); re-captures the waves."""
        for g in self.groups:
            g.eng.set_trace(on)
        self.record_packings = bool(on)
        self._packings = []
        self.invalidate_graph()

    def set_record_best(self, on=True, playout_incumbents=False):
        """Switches the incumbents of every group between pools (refused while episodes are being played); re-captures the waves.
        playout_incumbents: the playouts of evaluator="rollout" are candidates too (ValueError with `on` false or another evaluator);
        switching the incumbents off switches it off.  Off under move_rule MOVE_INCUMBENT: ValueError (switch the rule first)."""
        if not on and self.move_rule == _lib.MOVE_INCUMBENT:
            raise ValueError("move_rule MOVE_INCUMBENT is in force and follows the incumbents: set_move_rule to another rule first")
        if playout_incumbents and not (on and self.evaluator == "rollout"):
            raise ValueError("playout_incumbents needs record_best on and evaluator='rollout'")
        for g in self.groups:
            g.eng.set_incumbent(on)
            if on:
                g.eng.set_incumbent_playouts(playout_incumbents)
        self.record_best = bool(on)
        self.playout_incumbents = bool(playout_incumbents)
        self._best = []
        self.invalidate_graph()

    # ---- whole pools -------------------------------------------------------------------------------
    def _blocks(self, n):
        """Contiguous block of the pool per group: [(lo, hi)]; instance i has episode id first_id + i."""
        k = len(self.groups)
        base, rem = divmod(int(n), k)
        out, lo = [], 0
        for g in range(k):
            hi = lo + base + (1 if g < rem else 0)
            out.append((lo, hi)); lo = hi
        return out

    def _set_meta(self, g, lo, hi, episode_ids, thresholds):
        """Per-instance episode ids / R2 thresholds (bl [n], has_buf [n]) of group g's block lo:hi (rp_set_instance_meta)."""
        if episode_ids is None and thresholds is None:
            return
        ids = None if episode_ids is None else np.asarray(episode_ids, dtype=np.uint64)[lo:hi]
        bl = has = None
        if thresholds is not None:
            bl = np.asarray(thresholds[0], dtype=np.float64)[lo:hi]
            has = np.asarray(thresholds[1])[lo:hi]
        g.eng.set_instance_meta(ids, bl, has)

    def _set_initial(self, g, lo, hi, initial):
        """Initial states (rows [n, H], remaining [n, N], max_h [n] or None) of group g's block lo:hi (rp_set_instance_initial)."""
        if initial is None:
            return
        rows, rem, max_h = initial
        g.eng.set_instance_initial(rows[lo:hi], rem[lo:hi], None if max_h is None else max_h[lo:hi])

    def _check_initial(self, n, initial_rows, initial_remaining, max_h):
        """-> (rows uint64 [n, H], remaining uint8 [n, N], max_h int32 [n] or None), or None without an initial state."""
        if initial_rows is None and initial_remaining is None:
            if max_h is not None:
                raise ValueError("max_h belongs to an initial state: give initial_rows / initial_remaining")
            return None
        rows = np.zeros((n, self.H), np.uint64) if initial_rows is None else np.ascontiguousarray(initial_rows, dtype=np.uint64)
        rem = np.ones((n, self.N), np.uint8) if initial_remaining is None else (np.asarray(initial_remaining) != 0).astype(np.uint8)
        if rows.shape != (n, self.H) or rem.shape != (n, self.N):
            raise ValueError("initial_rows must be [n, H] and initial_remaining [n, N]")
        if max_h is not None:
            max_h = np.ascontiguousarray(max_h, dtype=np.int32).reshape(-1)
            if len(max_h) != n:
                raise ValueError("max_h needs one entry per instance")
        return rows, rem, max_h

    @staticmethod
    def _check_meta(n, episode_ids, thresholds):
        if episode_ids is not None and len(episode_ids) != n:
            raise ValueError("episode_ids needs one id per instance")
        if thresholds is not None and (len(thresholds) != 2 or len(thresholds[0]) != n or len(thresholds[1]) != n):
            raise ValueError("thresholds must be (bl [n], has_buf [n])")

    def _start(self, n, set_block, items, rewards_list, first_id, episode_ids, thresholds, initial_rows=None, initial_remaining=None, max_h=None):
        """start() and start_from_seeds(): set_block(g, lo, hi) sets group g's block lo:hi of the n instances as its engine's pool;
        items is what pop_packings needs to give the item sizes back."""
        buf = np.asarray(list(rewards_list), dtype=np.float64)
        self.first_id = int(first_id)
        self.n_instances = n
        self._check_meta(n, episode_ids, thresholds)
        initial = self._check_initial(n, initial_rows, initial_remaining, max_h)
        self._pool_items = (episode_ids, items) if self.record_packings or self.record_best else None
        self._pool_initial = initial
        torch.cuda.synchronize(self.device)  # the evaluator's weights may just have been trained on another stream
        if self.host_evaluator is None and self.fuse_elementwise and self.dense_small_convs:
            self.nnet.refresh_fused()
            torch.cuda.synchronize(self.device)
        for g, (lo, hi) in zip(self.groups, self._blocks(n)):
            if self.host_evaluator is None and self.evaluator == "cnn":
                with torch.cuda.stream(g.stream):
                    g.refresh_weights(self.nnet)  # stem tables follow in-place weight updates
            g.eng.set_rank_buffer(buf)
            set_block(g, lo, hi)
            self._set_meta(g, lo, hi, episode_ids, thresholds)
            self._set_initial(g, lo, hi, initial)
            g.eng.begin_pool()

    def start(self, item_wh, total_area, rewards_list=(), first_id=0, episode_ids=None, thresholds=None, initial_rows=None,
              initial_remaining=None, max_h=None):
        """The pool is cut into one contiguous block per group; instance i's episode id is first_id + i, or episode_ids[i].
        thresholds: (bl [n], has_buf [n]) -- instance i is ranked against that R2 threshold instead of rewards_list's.
        initial_rows uint64 [n, H] / initial_remaining uint8 [n, N]: instance i starts from that state instead of the empty bin with
        all items (rp_set_instance_initial; one of the two may be None: the empty bin / all items); total_area then includes the cells
        already set.  max_h [n]: the episode's max_h where the default -- the largest h of the items that take part -- is not it."""
        item_wh = np.ascontiguousarray(item_wh, dtype=np.uint8)
        total_area = np.ascontiguousarray(total_area, dtype=np.int32)
        self._start(item_wh.shape[0],
                    lambda g, lo, hi: g.eng.set_instance_pool(np.ascontiguousarray(item_wh[lo:hi]), np.ascontiguousarray(total_area[lo:hi]), self.first_id + lo),
                    item_wh, rewards_list, first_id, episode_ids, thresholds, initial_rows, initial_remaining, max_h)

    def start_from_seeds(self, seeds, rewards_list=(), first_id=0, bin_h=None, bin_w=None, episode_ids=None, thresholds=None, initial_rows=None,
                         initial_remaining=None, max_h=None):
        """Like start(), with instance i = ItemsGenerator.items_generator(seeds[i]) of the bin_w x bin_h rectangle (default: the
        board) generated on the device (rp_set_instance_pool_seeds: bit-identical to the host generator, tests/test_gpu_rules.py);
        total area bin_w * bin_h.  Seeded instances tile the bin, so they start from the empty bin: an initial state is refused."""
        if initial_rows is not None or initial_remaining is not None or max_h is not None:
            raise ValueError("a pool of generator seeds starts from the empty bin with all items: pass item_wh to start() for initial states")
        seeds = np.ascontiguousarray(seeds, dtype=np.uint32).reshape(-1)
        bin_w, bin_h = bin_w or self.W, bin_h or self.H
        self._start(seeds.shape[0],
                    lambda g, lo, hi: g.eng.set_instance_pool_seeds(np.ascontiguousarray(seeds[lo:hi]), bin_w, bin_h, self.first_id + lo),
                    (seeds, bin_w, bin_h), rewards_list, first_id, episode_ids, thresholds)

    def active(self):
        n = 0
        for g in self.groups:
            ph, _, _, _ = g.eng.status()
            n += int(np.isin(ph, (_lib.PHASE_RUNNING, _lib.PHASE_WAIT_EVAL, _lib.PHASE_MOVE_READY)).sum())
        return n

    def pop_finished(self):
        """(episode ids, outcomes, scores, moves) of the episodes finished since the last call, sorted by id.  With record_packings
        their layouts are set aside for pop_packings(), with record_best their incumbents for pop_best_packings()."""
        parts, best = [], []
        for g in self.groups:
            rec = g.eng.pop_finished(packings=self.record_packings, best=self.record_best)
            if self.record_best:
                best.append(rec[-1]); rec = rec[:-1]
            parts.append((rec[0].astype(np.int64),) + tuple(rec[1:]))
        ids = np.concatenate([p[0] for p in parts]); order = np.argsort(ids, kind="stable")
        out = tuple(np.concatenate([p[j] for p in parts])[order] for j in range(len(parts[0])))
        if self.record_packings and len(ids):
            self._keep_packings(*out)
        if self.record_best and len(ids):
            self._keep_best(out[0], {k: np.concatenate([b[k] for b in best])[order] for k in best[0]})
        return out[:4]

    def _pool_lookup(self):
        """-> (item sizes [n, N, 2] of the current pool, {episode id: instance index})."""
        if self._pool_items is None:
            raise RuntimeError("episodes finished before a pool was started with record_packings or record_best on")
        episode_ids, items = self._pool_items
        if isinstance(items, tuple):  # a pool of generator seeds: the same device generator gives the sizes back
            seeds, bin_w, bin_h = items
            items = self.eng.generate_items(seeds, bin_w=bin_w, bin_h=bin_h)
            self._pool_items = (episode_ids, items)
        pool_ids = self.first_id + np.arange(self.n_instances, dtype=np.int64) if episode_ids is None else np.asarray(episode_ids, dtype=np.int64)
        return items, {int(e): k for k, e in enumerate(pool_ids)}

    def _keep_best(self, ids, best):
        """Incumbents of finished episodes of the current pool as Packings.  The device keeps an incumbent's actions and final bin only;
        the rows every move filled are replayed on the host (solve.replay_rows) and the replay must end on the device's bin."""
        from .solve import Packing, replay_rows
        items, index = self._pool_lookup()
        initial = self._pool_initial
        for k in range(len(ids)):
            m, i = int(best["moves"][k]), index[int(ids[k])]
            start = {} if initial is None else dict(initial_board=initial[0][i], present=initial[1][i] != 0)
            actions = best["action"][k, :m].astype(np.int32)
            rows, board = replay_rows(self.W, self.H, items[i], actions, start.get("initial_board"))
            if not np.array_equal(board, best["board"][k]):
                raise RuntimeError("episode %d: the incumbent's actions replay to another bin than the engine recorded" % int(ids[k]))
            p = Packing(int(ids[k]), self.W, items[i], actions, rows, board, int(best["outcome"][k]), float(best["score"][k]), **start)
            p.prefix, p.updates = int(best["prefix"][k]), int(best["updates"][k])
            if "playout" in best:  # playout incumbents: where the record came from
                p.tree_moves, p.playout = int(best["tree_moves"][k]), int(best["playout"][k])
            self._best.append(p)

    def _keep_packings(self, ids, outcome, score, moves, action, rows, board):
        """Packing records of finished episodes of the current pool (their item sizes come from it)."""
        from .solve import Packing
        items, index = self._pool_lookup()
        initial = self._pool_initial
        for k in range(len(ids)):
            m, i = int(moves[k]), index[int(ids[k])]
            start = {} if initial is None else dict(initial_board=initial[0][i], present=initial[1][i] != 0)
            self._packings.append(Packing(int(ids[k]), self.W, items[i], action[k, :m], rows[k, :m], board[k], int(outcome[k]), float(score[k]), **start))

    def pop_packings(self):
        """solve.Packing of every episode that finished (and was popped: run() does) since the last call, sorted by episode id."""
        out = sorted(self._packings, key=lambda p: p.episode_id)
        self._packings = []
        return out

    def pop_best_packings(self):
        """The incumbent of every episode that finished (and was popped: run() does) since the last call as a solve.Packing with
        `prefix` and `updates` set, sorted by episode id (record_best)."""
        out = sorted(self._best, key=lambda p: p.episode_id)
        self._best = []
        return out

    def arena_peak(self):
        peaks = [g.eng.arena_peak() for g in self.groups]
        return {k: max(pk[k] for pk in peaks) for k in peaks[0]}

    def counters(self, reset=False):
        tot = dict.fromkeys(_lib.COUNTER_NAMES, 0)
        for g in self.groups:
            for name, val in g.eng.counters(reset=reset).items():
                tot[name] += val
        return tot

    def run(self, item_wh, total_area, rewards_list=(), first_id=0, poll=16, max_steps=None, episode_ids=None, thresholds=None,
            initial_rows=None, initial_remaining=None, max_h=None):
        """Plays every instance of the pool to the end.  Returns (episode ids, outcomes, scores, moves) sorted by id,
        plus timing / counter statistics.  episode_ids / thresholds / initial_rows / initial_remaining / max_h: see start()."""
        self.start(item_wh, total_area, rewards_list, first_id, episode_ids, thresholds, initial_rows, initial_remaining, max_h)
        return self._play_out(poll, max_steps)

    def run_from_seeds(self, seeds, rewards_list=(), first_id=0, bin_h=None, poll=16, max_steps=None, bin_w=None, episode_ids=None,
                       thresholds=None):
        """run() on device-generated instances (start_from_seeds)."""
        self.start_from_seeds(seeds, rewards_list, first_id, bin_h, bin_w, episode_ids, thresholds)
        return self._play_out(poll, max_steps)

    def _play_out(self, poll, max_steps):
        t0 = time.time()
        steps0 = self.steps
        while self.active() > 0:
            for _ in range(poll):
                self.step()
            if max_steps is not None and self.steps - steps0 >= max_steps:
                break
        torch.cuda.synchronize(self.device)
        dt = time.time() - t0
        ids, outcome, score, moves = self.pop_finished()
        stats = self.counters()
        stats.update(seconds=dt, steps=self.steps - steps0, episodes_finished=len(ids))
        return ids, outcome, score, moves, stats

    # ---- replay ---------------------------------------------------------------------------------
    def examples_packed(self):
        """Everything recorded so far as ONE PackedReplay (replay.py: ~0.4 KB per example) in the reference's order: episode by
        episode, move by move (CoachBPP.py:80,133) -- the device buffers themselves fill in completion order across slots."""
        from .replay import PackedReplay
        torch.cuda.synchronize(self.device)
        parts = [PackedReplay.from_engine(g.eng, self.device) for g in self.groups]
        torch.cuda.synchronize(self.device)  # the copies ran on the groups' streams
        return PackedReplay.cat(parts).sort_by_episode_move()

    def examples(self, with_meta=False):
        """(planes [E, N+1, H, W], pi [E, A], value [E]) float32 device tensors of everything recorded so far, in the reference's
        order -- the packed set expanded once (small pools, tests; training expands per minibatch instead).
        with_meta: also (episode ids [E] int64, move numbers [E] int32) as numpy arrays."""
        rep = self.examples_packed()
        res = rep.dense()
        torch.cuda.synchronize(self.device)
        return res + (rep.episode.cpu().numpy(), rep.move.cpu().numpy()) if with_meta else res

    def clear_examples(self):
        for g in self.groups:
            g.eng.examples_clear()
