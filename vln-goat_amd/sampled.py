"""Sampled walks of a dagger iteration (overview: rollout.py): the policy's own walk, decided step by step from step graphs
replayed over the buffers of a `TeacherEpisode` (episodes.py).  The top layer: only the rollout.py façade imports this module.

  * `SampledEpisode`              pass 1 of the two-pass form (M/r2r/agent.py:436-437,575-607): captured FORWARD graphs decide the
                                  walk; the finished plan then goes through the captured forward + backward body.
  * `ArgmaxEpisode`               the validation walk (feedback = 'argmax'): the same step graphs in eval mode, the argmax, the stop score
                                  and the best object of a step in one read-back; stop-node backtrack and `pred_objid` on the host.
  * `SinglePassSampledEpisode`    the reference's one-pass form (M/r2r/agent.py:596-690): the step graphs keep their autograd state
                                  and ONE captured backward graph differentiates the loss through all of them."""
import gc
import time
import warnings

import numpy as np
import torch

from . import hipops
from .episodes import EpisodePlanner


def _sampled_walk(ep, episodes, rng, sampler, replay_all):
    """The walk both sampled forms drive over their graphs (ep.g_lang, ep.g_step, ep.probs): per step build the tables, copy them
    into the buffers, replay, read the B x G probabilities back, sample.  -> (planner, actions); sets ep.host_s (seconds in the host
    builders) and ep.steps.  replay_all=False: stops once every episode has ended (the planner is then short of te.T steps).
    True: every step graph is replayed; behind the end a step runs on ignore labels, without a read-back."""
    te, bufs = ep.te, ep.bufs
    rng = rng if rng is not None else np.random.RandomState(0)
    t0 = time.perf_counter()
    p = EpisodePlanner(te, episodes, imitation=False)
    ep.host_s = time.perf_counter() - t0
    bufs.load_part({'txt_ids': p.out['txt_ids'], 'txt_masks': p.out['txt_masks']})
    ep.g_lang.replay()
    actions, zeros = [], np.zeros(len(episodes), np.int64)
    for t in range(te.T):
        t0 = time.perf_counter()
        part = p.build_step()
        ep.host_s += time.perf_counter() - t0
        bufs.load_part(part)
        ep.g_step[t].replay()
        if p.ended.all():                                 # (replay_all) nothing left to decide
            a = zeros
        else:
            probs = ep.probs[t].cpu().numpy()             # (synchronises: the step's one read-back)
            a = np.asarray(sampler(t, probs), np.int64) if sampler is not None else SampledEpisode.sample(probs, rng)
            a = np.where(p.ended, 0, a)
            actions.append(a)
        t0 = time.perf_counter()
        p.advance(a)
        ep.host_s += time.perf_counter() - t0
        if p.ended.all() and not replay_all:
            break
    ep.steps = len(actions)
    return p, actions


class SampledEpisode:
    """Pass 1 of the two-pass sampled rollout (feedback = 'sample': M/r2r/agent.py:436-437,575-607) as captured FORWARD graphs over
    the buffers of a TeacherEpisode: one graph for the instruction and its K|V projections, one per step t (feature gather, panorama
    encoder, node-embedding gather over the panoramas of the steps <= t, navigation step, softmax).  Nothing is differentiated here:
    the pass only decides the walk.  Per step the host builds the step's tables from the navigator's state (EpisodePlanner.build_step),
    copies them into the episode buffers (one small pinned H2D), replays the step graph, reads the B x G action probabilities back — the
    one device -> host copy of the step — and samples.  run() returns the finished plan (== TeacherEpisode.plan(episodes, actions):
    the walk the policy took, the DAgger labels of its states), ready for `bufs.load(plan)` + the captured forward + backward body.

        se = SampledEpisode(te, model, bufs, extras)              # captures T + 1 small graphs (bufs holds any valid plan)
        plan, actions = se.run(episodes, rng);  bufs.load(plan);  episode_graph.replay()"""

    def __init__(self, te, model, bufs, extras=None, bump_masks=True):
        """bump_masks=False: the step graphs do not advance the device-side dropout counter (they read whatever it holds): for running
        this pass BESIDE a training graph on another stream — a bump between that graph's forward and backward kernels would make its
        backward regenerate other masks than its forward drew; a forward-only pass needs no particular counter value."""
        self.te, self.bufs = te, bufs
        extras = extras or {}
        t_ = bufs.t
        B = t_['txt_ids'].shape[0]

        def fresh_masks():                  # (a replay draws new dropout masks: the in-graph bump of the device-side counter, if one is in use)
            if bump_masks and hipops.RngState.dev is not None:
                hipops.RngState.dev.add_(0x9E3779B1)

        def language():
            fresh_masks()
            return te._instruction(model, t_, extras, False)       # (forward only: no autograd handles)
        self.g_lang, (self.txt, self.txt_kv) = self._capture(language)
        nav_extras = te._nav_extras(extras, self.txt.dtype)
        self.g_step, self.probs = [], []
        pool, last = [], None
        for s in range(te.T):
            def step(s=s, pool=pool, last=last):
                fresh_masks()
                mine = list(pool)
                pano, pmask, fused = te._panoramas(model, t_, extras, 's%d_' % s, B, B)
                logits, new_last, _ = te._nav_step(model, t_, s, self.txt, self.txt_kv, pano, pmask, fused, mine, last, nav_extras)
                return torch.softmax(logits.float(), 1), mine, new_last
            g, (probs, pool, last) = self._capture(step)
            self.g_step.append(g)
            self.probs.append(probs)
        self._keep = (pool, last)               # (the static outputs the later step graphs read)
        self.host_s = 0.0

    @staticmethod
    def _capture(fn):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side), torch.no_grad():
            fn()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.no_grad(), hipops.graph(g):
            out = fn()
        return g, out

    @staticmethod
    def sample(probs, rng):
        """Categorical(probs).sample() on the host: inverse CDF per row (rows are the B episodes; never a zero-probability node)."""
        c = np.cumsum(probs.astype(np.float64), 1)
        # u < c[-1] strictly (a product that rounds up to c[-1] would select the slot behind the last node with probability mass —
        # a padding slot, which advance() rejects): the first index whose cumulative mass exceeds u always has probs > 0
        u = np.minimum(rng.random_sample(probs.shape[0]) * c[:, -1], np.nextafter(c[:, -1], 0.0))
        return np.array([int(np.searchsorted(c[i], u[i], side='right')) for i in range(probs.shape[0])], np.int64)

    def run(self, episodes, rng=None, sampler=None):
        """-> (plan, actions).  sampler(t, probs [B, G] numpy) -> actions [B] overrides the random draw (tests: a fixed action sequence)."""
        p, actions = _sampled_walk(self, episodes, rng, sampler, replay_all=False)
        t0 = time.perf_counter()
        while p.t < self.te.T:                                     # every episode has ended: the remaining steps carry no label
            p.build_step()
            p.advance(np.zeros(len(episodes), np.int64))
        plan = p.finish()
        self.host_s += time.perf_counter() - t0
        return plan, actions


class ArgmaxEpisode:
    """The validation walk (feedback = 'argmax': M/r2r/main_nav.py `valid` -> agent.test(), M/r2r/agent.py:575-672) as captured step
    graphs over the buffers of a TeacherEpisode: the instruction graph and T step graphs of SampledEpisode, captured under no_grad with
    the model in EVAL mode (an nn.Module's training flag is put back afterwards; a plain callable is taken as it is).  Each step graph
    ends by writing [argmax, softmax[:, 0], best object index] into one static [3, B] float32 tensor with the torch ops NavRollout.run
    uses — the step's only device -> host copy.  The host side (EpisodePlanner(feedback='argmax')) applies the argmax stop rule, records
    the stop scores, appends the backtrack to the best stop node and fills `pred_objid`, exactly as NavRollout.run(feedback='argmax').

        walk = ArgmaxEpisode(te, model, bufs, extras)             # captures T + 1 small graphs (bufs holds any valid plan)
        traj = walk.run(episodes)                                  # [{'instr_id', 'path': [[vp], hop, ...], 'pred_objid'}]

    The object holds no autograd state: it may be built before or after, and live beside, the training graphs of the process (TeacherEpisode
    bodies, SampledEpisode) — unlike SinglePassSampledEpisode, whose step graphs keep their autograd graph alive and which therefore cannot
    coexist with a second instance or a later training-step capture.  It shares `bufs` with whatever else replays over them: run() rewrites
    the step tables, so load the training plan again before the next training replay."""

    def __init__(self, te, model, bufs, extras=None):
        self.te, self.bufs = te, bufs
        extras = extras or {}
        t_ = bufs.t
        self.B = B = t_['txt_ids'].shape[0]
        has_obj = te.objects is not None
        self.back = torch.zeros(3, B, dtype=torch.float32, device=t_['txt_ids'].device)
        module = model if isinstance(model, torch.nn.Module) else None
        was_training = module.training if module is not None else False
        if module is not None:
            module.eval()
        try:
            self.g_lang, (self.txt, self.txt_kv) = SampledEpisode._capture(lambda: te._instruction(model, t_, extras, False))
            nav_extras = te._nav_extras(extras, self.txt.dtype)
            self.g_step = []
            pool, last = [], None
            for s in range(te.T):
                def step(s=s, pool=pool, last=last):
                    mine = list(pool)
                    pano, pmask, fused = te._panoramas(model, t_, extras, 's%d_' % s, B, B)
                    logits, new_last, obj_logits = te._nav_step(model, t_, s, self.txt, self.txt_kv, pano, pmask, fused, mine, last, nav_extras)
                    probs = torch.softmax(logits.detach().float(), 1)
                    rows = [probs.argmax(1).to(torch.float32), probs[:, 0].detach()]
                    if has_obj:                 # the best object of every sample's current viewpoint (M/reverie/agent_obj_goat.py:680-690)
                        vl = t_['s%d_view_lens' % s]
                        pos = torch.arange(obj_logits.shape[1], device=obj_logits.device)[None, :]
                        ol = torch.where(pos >= (vl + 2)[:, None], obj_logits.detach().float(), torch.full_like(obj_logits, -float('inf'), dtype=torch.float32))
                        rows.append((ol.argmax(1) - (vl + 2)).to(torch.float32))
                    else:
                        rows.append(torch.zeros_like(rows[1]))
                    self.back.copy_(torch.stack(rows, 0))
                    return mine, new_last
                g, (pool, last) = SampledEpisode._capture(step)
                self.g_step.append(g)
            self._keep = (pool, last)               # (the static outputs the later step graphs read)
        finally:
            if module is not None:
                module.train(was_training)
        self.host_s, self.steps, self.actions = 0.0, 0, []

    def run(self, episodes, navigator=None, check_every=None):
        """-> the trajectories of the argmax walk, one per episode: {'instr_id', 'path', and with objects 'pred_objid'}.
        navigator: a navdev.DeviceNavigator(te, tables, bufs, 'argmax') — the walk is then T navigator launches and T graph replays
        with one read-back at its end (every step graph is replayed; an ended episode's rows stay frozen).  check_every=k: the host
        reads the number of live episodes every k steps and stops replaying once it is zero (DeviceNavigator.walk)."""
        te, bufs = self.te, self.bufs
        if len(episodes) != self.B:
            raise ValueError('ArgmaxEpisode: %d episodes for graphs captured at B = %d' % (len(episodes), self.B))
        if navigator is not None:
            traj, self.actions, _, _ = navigator.walk(self, episodes, act=lambda t: self.back, check_every=check_every)
            self.host_s, self.steps = navigator.host_s, len(self.actions)
            return traj
        t0 = time.perf_counter()
        p = EpisodePlanner(te, episodes, imitation=False, feedback='argmax')
        self.host_s = time.perf_counter() - t0
        bufs.load_part({'txt_ids': p.out['txt_ids'], 'txt_masks': p.out['txt_masks']})
        self.g_lang.replay()
        self.actions = []
        for t in range(te.T):
            t0 = time.perf_counter()
            part = p.build_step()
            self.host_s += time.perf_counter() - t0
            bufs.load_part(part)
            self.g_step[t].replay()
            back = self.back.cpu().numpy()                    # (synchronises: the step's one read-back)
            a = np.where(p.ended, 0, back[0].astype(np.int64))
            self.actions.append(a)
            t0 = time.perf_counter()
            p.advance(a, back[1], back[2] if te.objects is not None else None)
            self.host_s += time.perf_counter() - t0
            if p.ended.all():
                break
        self.steps = len(self.actions)
        return p.traj


class SinglePassSampledEpisode:
    """The sampled half of a dagger iteration in ONE pass, as the reference runs it (M/r2r/agent.py:596-690: the action is sampled at
    :629-633 from the SAME forward whose logits carry the loss), at graph speed: the instruction graph and the T step graphs of
    SampledEpisode captured WITH their autograd state kept alive (activations stay in the graphs' shared memory pool), and ONE captured
    backward graph that forms the loss over the logits the steps left behind — the DAgger labels of the visited states are part of each
    step's tables — and differentiates it through all T steps ([MEM] state, node-embedding pool, the instruction's K|V bank).  Against the
    two-pass form (SampledEpisode + the episode graph) the forward of pass 2 is gone, and the walk and the gradient see the same dropout
    masks (sample-equivalent to the eager single pass, not only distribution-equivalent).

        sp = SinglePassSampledEpisode(te, model, bufs, extras, prologue=lambda: arena.zero('nav'))
        traj, actions = sp.run(episodes, rng)          # gradients of the sampled loss are in the arena / .grad; sp.loss holds its value

    Dropout: the device-side counter is bumped ONCE per iteration (instruction graph); every op of every step draws from its own counter
    range, and the backward graph regenerates the masks from the same counter value.  Every step graph is replayed in every iteration (an
    ended episode's rows carry the ignore label): no graph ever differentiates through buffers it has not written.
    As for every capture of a training step: no tensor of an EARLIER backward pass (a loss, logits kept on an object) may be alive when
    this object is built — it would keep AccumulateGrad nodes bound to the eager stream alive and the captured backward would accumulate
    outside the capture (hipops.graph raises; on ROCm 7.2 ending that capture can also crash the process).
    That holds for this class's own instances too: `_keep` holds the steps' logits WITH their grad_fn (the backward graph reads them),
    so the captured autograd graph lives as long as the object.  ONE live instance at a time (no second (B, T) bucket beside it),
    built AFTER every TeacherEpisode training graph of the process; a second instance or a later training-step capture raises the
    RuntimeError of the warm-up below."""

    def __init__(self, te, model, bufs, extras=None, prologue=None, loss_scale=1.0):
        self.te, self.bufs = te, bufs
        extras = extras or {}
        t_ = bufs.t
        B, T = t_['txt_ids'].shape[0], te.T

        def language():
            if prologue is not None:
                prologue()
            if hipops.RngState.dev is not None:
                hipops.RngState.dev.add_(0x9E3779B1)
            return te._instruction(model, t_, extras, True)        # (txt_h, kv_h: one autograd handle per step)

        def step(s, txt_h, kv_h, pool, last, nav_extras):
            mine = list(pool)
            pano, pmask, fused = te._panoramas(model, t_, extras, 's%d_' % s, B, B)
            logits, new_last, obj_logits = te._nav_step(model, t_, s, txt_h[s], kv_h[s], pano, pmask, fused, mine, last, nav_extras)
            with torch.no_grad():
                probs = torch.softmax(logits.detach().float(), 1)
            return probs, mine, new_last, logits, obj_logits

        def backward(logits, obj_logits):
            rows = []
            for s in range(T):
                rows += te._loss_rows(t_, s, logits[s], obj_logits[s])
            loss = torch.stack(rows, 0).sum() / B
            (loss * loss_scale if loss_scale != 1.0 else loss).backward()
            return loss.detach()

        def whole():
            txt_h, kv_h = language()
            nav_extras = te._nav_extras(extras, txt_h[0].dtype)
            pool, last, lg, og = [], None, [], []
            for s in range(T):
                _, pool, last, l, o = step(s, txt_h, kv_h, pool, last, nav_extras)
                lg.append(l)
                og.append(o)
            return backward(lg, og)

        # eager warm-up of the whole chain (weight shadows, kernel attributes, GEMM tuning where the tuner is on) with the parallel branches
        # forked as the captures will fork them; nothing of it may outlive into the captures (hipops.graph raises on a live warm-up graph)
        # A tensor of an EARLIER backward pass that is still alive shows up right here, as torch's AccumulateGrad stream-mismatch warning (the
        # warm-up runs on a stream of its own): raised as an error BEFORE anything is captured — inside the capture the same condition ends in
        # a crash of hipStreamEndCapture on ROCm 7.2, not in an exception.
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        always = torch.is_warn_always_enabled()
        torch.set_warn_always(True)                 # (torch emits this warning ONCE per process otherwise: an earlier, harmless occurrence would hide this one)
        with warnings.catch_warnings():
            warnings.filterwarnings('error', message=".*AccumulateGrad node's stream does not match.*")
            try:
                with torch.cuda.stream(side), hipops.Branch.like_capture():
                    whole()
            except UserWarning as e:
                torch.cuda.current_stream().wait_stream(side)
                torch.cuda.synchronize()
                hipops.WgradQueue.reset()
                raise RuntimeError('SinglePassSampledEpisode: an autograd graph of an earlier pass is still alive (a loss / logits tensor kept '
                                   'somewhere): its AccumulateGrad nodes are bound to that pass\'s stream and a captured backward would accumulate '
                                   'outside the capture.  Release those tensors (del, gc.collect()) before building this object.') from e
            finally:
                torch.set_warn_always(always)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        gc.collect()

        self._pool = None
        self.g_lang, (txt_h, kv_h) = self._capture(language)
        nav_extras = te._nav_extras(extras, txt_h[0].dtype)
        self.g_step, self.probs = [], []
        pool, last, lg, og = [], None, [], []
        for s in range(T):
            g, (probs, pool, last, l, o) = self._capture(lambda s=s, pool=pool, last=last: step(s, txt_h, kv_h, pool, last, nav_extras))
            self.g_step.append(g)
            self.probs.append(probs)
            lg.append(l)
            og.append(o)
        self.g_bwd, self.loss = self._capture(lambda: backward(lg, og))
        self._keep = (txt_h, kv_h, pool, last, lg, og)         # (the static tensors the graphs read)
        torch.cuda.synchronize()
        self.host_s, self.steps = 0.0, 0

    def _capture(self, fn):
        g = torch.cuda.CUDAGraph()
        with hipops.graph(g, **({} if self._pool is None else {'pool': self._pool})):
            out = fn()
        self._pool = g.pool()
        return g, out

    def run(self, episodes, rng=None, sampler=None, navigator=None):
        """-> (trajectories, actions).  The parameter gradients of the sampled loss are where the model's backward puts them (the gradient
        arena / .grad) when this returns (asynchronously: on the current stream); `self.loss` is the loss of the iteration (device scalar).
        sampler(t, probs [B, G] numpy) -> actions [B] overrides the random draw (tests: a fixed action sequence).
        navigator: a navdev.DeviceNavigator(te, tables, bufs, 'sample') — the walk is decided on the device from the same uniforms
        (`rng.random_sample((T, B))`), with no read-back before the backward graph has been launched; returns after the one read-back."""
        if navigator is not None:
            if sampler is not None:
                raise ValueError('SinglePassSampledEpisode: a sampler decides on the host; the device navigator samples itself')
            traj, actions, self.n_traj, _ = navigator.walk(self, episodes, rng=rng, act=lambda t: self.probs[t], after=self.g_bwd.replay)
            self.host_s, self.steps = navigator.host_s, len(actions)
            return traj, actions
        p, actions = _sampled_walk(self, episodes, rng, sampler, replay_all=True)
        self.g_bwd.replay()
        self.n_traj = p.n_traj
        return p.traj, actions
