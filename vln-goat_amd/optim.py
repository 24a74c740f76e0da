"""Fused optimizer step on the gradient arena: the update either side of the forward/backward path.

Reference behaviour (P = /root/reference/pretrain_src):
  * P/optim/misc.py:13-37    build_optimizer: two parameter groups by NAME — weight decay for everything except names
                             containing 'bias', 'LayerNorm.bias', 'LayerNorm.weight' — lr / betas from the options
  * P/optim/adamw.py:53-110  HF-style AdamW: bias-corrected step size from the PARAMETER's own step count, decoupled decay
                             applied after the update, parameters whose .grad is None skipped (no moment update, no decay)
  * P/train_r2r_goat.py:349-366   per update: lr of the schedule into every group, clip_grad_norm_(5.0), optimizer.step()
Here the gradients already sit in ONE float32 buffer (dp.GradArena); the moments get two buffers of the same layout and the
whole update is two kernels (goat_grad_sqnorm, goat_adamw_step in csrc/optim.hip) that also refresh the bf16 operand
"shadows" of the weights, so the next forward needs no cast kernels.  No host synchronisation: the clip coefficient is
computed on the device; `last_grad_norm()` reads it back on request.

Fine-tuning (M = the reference's map_nav_src) ends its iteration with another update — FusedTorchOptim below:
  * M/r2r/agent_base.py:105-123    torch.optim.{RMSprop | Adam | AdamW | SGD}(vln_bert.parameters(), lr=args.lr), torch's defaults; a second
                                   optimizer of the same class over the critic
  * M/r2r/agent_base.py:191-200    loss.backward(); clip_grad_norm_(vln_bert.parameters(), 40.); both .step(); the lr schedule's .step()
  * M/r2r/agent_base.py:205-253    optimizer.state_dict() saved / loaded with the checkpoint (--save_optimizer / --resume_optimizer)
"""
import ctypes

import torch

from . import _lib
from ._plumbing import _ptr, launch
from .shadows import BPAD, CAT, CATB, PLAIN, ROWPAD, key_kind, member_ids

NO_DECAY = ('bias', 'LayerNorm.bias', 'LayerNorm.weight')      # P/optim/misc.py:13
CHUNK = 65536


def _copies(plist):
    """Which cached operand copies the update kernel refreshes itself.  -> ({id(p): slots}, done) with slots =
    {'s0', 's1': bf16 pointers in the parameter's element order, 'cols', 'ld0': s0 is a row-padded image, 'f32': float32
    pointer} and done = the storage addresses of the copies that are COMPLETELY covered by the slots handed out (a
    concatenated copy only when each of its members got one).  Everything else is rebuilt in place after the kernel by
    hipops.refresh_shadows — a cached copy is never dropped: a captured hipGraph may read it at its address.
    (Key layouts: the table at the top of shadows.py.)"""
    by_id = {id(p): p for p in plist}
    slots = {id(p): {'bf16': [], 'pad': None, 'f32': None} for p in plist}
    whole = []            # (tensor, [(param id, kind, pointer)]) per cached copy
    for p in plist:
        cache = p.__dict__.get('_goat_shadow')
        if not cache:
            continue
        for k, (ver, t) in cache.items():
            if not t.is_contiguous():
                continue
            kd = key_kind(k)
            if kd == CAT:
                if k[1] != torch.bfloat16 or k[2] or any(i not in by_id for i in member_ids(k)):
                    continue
                row, members = 0, []
                for i in member_ids(k):
                    members.append((i, 'bf16', t.data_ptr() + row * t.shape[1] * 2))
                    row += by_id[i].shape[0]
                whole.append((t, members))
            elif kd == CATB:
                if t.dtype != torch.float32 or any(i not in by_id for i in member_ids(k)):
                    continue
                off, members = 0, []
                for i in member_ids(k):
                    members.append((i, 'f32', t.data_ptr() + off * 4))
                    off += by_id[i].numel()
                whole.append((t, members))
            elif kd == ROWPAD:
                if t.dtype == torch.bfloat16 and t.shape[1:] == p.shape[1:] and t.shape[0] >= p.shape[0]:
                    whole.append((t, [(id(p), 'bf16', t.data_ptr())]))
            elif kd == BPAD:          # zero-padded float32 image of a bias: the leading numel(p) floats are the bias
                if t.dtype == torch.float32 and t.numel() >= p.numel():
                    whole.append((t, [(id(p), 'f32', t.data_ptr())]))
            elif kd == PLAIN and k[0] == torch.bfloat16 and k[1] is False and t.dtype == torch.bfloat16:
                if k[2] == 0:
                    whole.append((t, [(id(p), 'bf16', t.data_ptr())]))
                elif p.dim() == 2:
                    whole.append((t, [(id(p), 'pad', (t.data_ptr(), p.shape[1], p.shape[1] + k[2]))]))
    done = set()
    for t, members in whole:
        ok = True
        for i, kind, _ in members:        # does every member still have a free slot of that kind?
            sl = slots[i]
            if kind == 'bf16':
                ok &= len(sl['bf16']) < (1 if sl['pad'] is not None else 2)
            elif kind == 'pad':
                ok &= sl['pad'] is None and len(sl['bf16']) < 2
            else:
                ok &= sl['f32'] is None
        if not ok:
            continue
        for i, kind, ptr in members:
            if kind == 'bf16':
                slots[i]['bf16'].append(ptr)
            else:
                slots[i][kind] = ptr
        done.add(t.data_ptr())
    return slots, done


def _task_key(task):
    return task.split('_')[0] if task is not None else None


class _Upload:
    """A block of device memory written from the host: staged through pinned memory and copied asynchronously on the current stream, so
    work launched after send() reads the new bytes and work launched before it the old ones.  The event orders the NEXT send() behind this
    copy's read of the pinned block (graph-replay loops never synchronise).  A CPU arena has no pinned memory: a plain copy."""

    def __init__(self, nbytes, dev):
        self.dev = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
        self._pinned = torch.zeros(nbytes, dtype=torch.uint8).pin_memory() if dev.type == 'cuda' else None
        self._copied = None

    def send(self, raw):
        if self._pinned is None:
            self.dev.copy_(raw)
            return
        if self._copied is not None:
            self._copied.synchronize()
        self._pinned.copy_(raw)
        self.dev.copy_(self._pinned, non_blocking=True)
        self._copied = torch.cuda.Event()
        self._copied.record()


class _Table:
    """What either update hands its kernels for the parameters among `ids` that the task `key` uses (every arena parameter of `ids` if
    None), in arena order: the chunk table, the arena ranges of the norm and the tensor table (`struct`: _lib.AdamwTensor or
    _lib.OptimTensor, which name the shared fields alike)."""

    def __init__(self, arena, ids, key, struct):
        self.arena = arena
        self.params = [p for p in arena.params if id(p) in ids and (arena.tasks_of[id(p)] is None or key is None or key in arena.tasks_of[id(p)])]
        chunks, rng = [], []
        for i, p in enumerate(self.params):
            for first in range(0, p.numel(), CHUNK):
                chunks += [i, first]
            a = arena.offsets[id(p)]
            rng += [a, a + p.numel()]        # the norm runs over the parameters' own elements (the alignment padding between arena slices is never written: zeros)
        dev = arena.flat.device
        self.chunks, self.nchunks = torch.tensor(chunks, dtype=torch.int32, device=dev), len(chunks) // 2
        self.ranges, self.n_ranges = torch.tensor(rng, dtype=torch.int64, device=dev), len(rng) // 2
        self.host = (struct * max(1, len(self.params)))()
        self.entries = list(self.host)[:len(self.params)]       # (views into `host`, made once: indexing a ctypes array builds a new object)
        self._upload = _Upload(ctypes.sizeof(self.host), dev)
        self.dev = self._upload.dev

    def fill(self):
        """the eight shared fields of every entry from the cached copies of now -> `done` of _copies()"""
        slots, done = _copies(self.params)
        for e, p in zip(self.entries, self.params):
            sl = slots[id(p)]
            e.param, e.arena_off, e.numel = p.data_ptr(), self.arena.offsets[id(p)], p.numel()
            bf = list(sl['bf16'])
            if sl['pad'] is not None:
                e.shadow0, e.cols, e.ld0 = sl['pad']
                e.shadow1 = bf[0] if bf else None
            else:
                e.cols, e.ld0 = 0, 0
                e.shadow0 = bf[0] if len(bf) > 0 else None
                e.shadow1 = bf[1] if len(bf) > 1 else None
            e.shadow_f32 = sl['f32']
        return done

    def send(self):
        nbytes = ctypes.sizeof(self.host)
        self._upload.send(torch.frombuffer((ctypes.c_uint8 * nbytes).from_address(ctypes.addressof(self.host)), dtype=torch.uint8))


class FusedAdamW:
    """optimizer over the parameters of a dp.GradArena.

        opt = FusedAdamW(model.named_parameters(), arena, lr=5e-5, betas=(0.9, 0.98), weight_decay=0.01)
        ... backward of `task` (gradients in the arena) ...
        opt.step(task, max_norm=5.0)

    `param_groups` mirrors the reference's two groups ({'lr', 'weight_decay', 'names'}) so that a trainer's
    `for g in optimizer.param_groups: g['lr'] = lr_this_step` keeps working."""

    def __init__(self, named_params, arena, lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.0, correct_bias=True):
        if lr < 0.0 or not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0 or eps < 0.0:
            raise ValueError('invalid AdamW hyper-parameters')                       # P/optim/adamw.py:44-51
        self.arena = arena
        self.betas, self.eps, self.correct_bias = (float(betas[0]), float(betas[1])), float(eps), bool(correct_bias)
        named = [(n, p) for n, p in named_params if id(p) in arena.views]
        self.names = {id(p): n for n, p in named}
        decay = [n for n, _ in named if not any(nd in n for nd in NO_DECAY)]
        no_decay = [n for n, _ in named if any(nd in n for nd in NO_DECAY)]
        self.param_groups = [{'lr': float(lr), 'weight_decay': float(weight_decay), 'names': decay},
                             {'lr': float(lr), 'weight_decay': 0.0, 'names': no_decay}]
        self._group_of = {n: 0 for n in decay}
        self._group_of.update({n: 1 for n in no_decay})
        dev = arena.flat.device
        self.exp_avg = torch.zeros_like(arena.flat)
        self.exp_avg_sq = torch.zeros_like(arena.flat)
        self.steps = {id(p): 0 for _, p in named}                                   # state['step'] of every parameter
        self._sq = torch.zeros(1, dtype=torch.float32, device=dev)
        self._tables = {}                # per task key (static): which tensors, their chunks, the arena ranges of the norm
        self._by_id = {id(p): p for _, p in named}
        self.last_refreshed = 0          # copies rebuilt by torch ops after the last step (0 in the steady bf16 state)

    def step(self, task=None, max_norm=5.0):
        """clip_grad_norm_(max_norm) + AdamW on the parameters `task` uses (all arena parameters if None)."""
        from . import hipops
        key = _task_key(task)
        tb = self._tables.get(key)
        if tb is None:
            tb = self._tables[key] = _Table(self.arena, self.names, key, _lib.AdamwTensor)
        if not tb.params:
            return
        arena = self.arena
        b1, b2 = self.betas
        done = tb.fill()
        for e, p in zip(tb.entries, tb.params):
            self.steps[id(p)] += 1
            t = self.steps[id(p)]
            g = self.param_groups[self._group_of[self.names[id(p)]]]
            lr = g['lr']
            e.step_size = lr * ((1.0 - b2 ** t) ** 0.5) / (1.0 - b1 ** t) if self.correct_bias else lr
            e.decay = lr * g['weight_decay']
        tb.send()
        self._sq.zero_()
        clip = max_norm is not None and max_norm > 0
        launch('goat_grad_sqnorm', arena.flat, tb.ranges, tb.n_ranges, self._sq)
        launch('goat_adamw_step', arena.flat, self.exp_avg, self.exp_avg_sq, tb.dev, tb.chunks, tb.nchunks, b1, b2, self.eps,
               float(max_norm) if clip else 0.0, self._sq)
        # the copies the kernel did not cover (transposed / float32 images of the parity mode, a third bf16 copy): same storage, new values
        by_id = self._by_id
        self.last_refreshed = sum(hipops.refresh_shadows(p, by_id, done) for p in tb.params)

    def last_grad_norm(self):
        """total gradient norm of the last step() (synchronises)."""
        return float(self._sq.sqrt().item())

    def state_of(self, p):
        a = self.arena.offsets[id(p)]
        return {'step': self.steps[id(p)], 'exp_avg': self.exp_avg[a:a + p.numel()].view_as(p), 'exp_avg_sq': self.exp_avg_sq[a:a + p.numel()].view_as(p)}


def build_optimizer(model, opts, arena):
    """P/optim/misc.py:11-37 on the arena: opts.optim must be 'adamw' (the shipped configuration); learning_rate, betas,
    weight_decay as there."""
    if getattr(opts, 'optim', 'adamw') != 'adamw':
        raise ValueError('invalid optimizer')
    return FusedAdamW(model.named_parameters(), arena, lr=opts.learning_rate, betas=tuple(opts.betas), weight_decay=opts.weight_decay)


# ---------------------------------------------------------------------------------------------------------------- fine-tuning
_TORCH_OPTIM = {'rms': ('RMSprop', _lib.OPT_RMSPROP), 'adam': ('Adam', _lib.OPT_ADAM), 'adamW': ('AdamW', _lib.OPT_ADAMW),
                'sgd': ('SGD', _lib.OPT_SGD)}                                      # args.optim, M/r2r/agent_base.py:108-117
_MOMENTS = {_lib.OPT_ADAMW: ('exp_avg', 'exp_avg_sq'), _lib.OPT_ADAM: ('exp_avg', 'exp_avg_sq'), _lib.OPT_RMSPROP: ('square_avg',),
            _lib.OPT_SGD: ()}                                                      # torch's state keys, in torch's order after 'step'
_UNSUPPORTED = ('momentum', 'centered', 'amsgrad', 'nesterov', 'dampening', 'maximize', 'capturable', 'differentiable')


class FusedTorchOptim:
    """torch.optim.{RMSprop | Adam | AdamW | SGD} + clip_grad_norm_ on the parameters of a dp.GradArena that `task` uses: the update
    the reference's fine-tuning iteration ends with (M/r2r/agent_base.py:105-123, 191-200).

        opt = FusedTorchOptim(vln_bert.named_parameters(), arena, algo=args.optim, lr=args.lr)
        ... the iteration's backward passes (gradients in the 'nav' arena) ...
        opt.step(max_norm=40.0)             # goat_grad_sqnorm, goat_optim_step, goat_optim_advance: three launches

    One parameter group with torch's keys (`param_groups[0]`), torch's formulas and defaults, torch's state_dict format.  Everything
    a step reads that changes between steps lives in device memory (learning rate and the other hyper-parameters, the step counter, the
    gradient norm), so `step()` inside `hipops.graph(g)` records device work only: between replays, `set_lr(x)` is the schedule.
    Parameters outside the arena (unused, frozen, requires_grad=False) are never touched and have no state."""

    def __init__(self, named_params, arena, algo='adamW', lr=1e-5, task='nav', **torch_defaults):
        if algo not in _TORCH_OPTIM:
            raise ValueError('invalid optimizer %r (rms | adam | adamW | sgd)' % (algo,))
        cls_name, self.algo = _TORCH_OPTIM[algo]
        self.torch_class = getattr(torch.optim, cls_name)
        # torch validates the hyper-parameters and supplies its defaults and group keys: the group of the installed torch, minus 'params'
        group = dict(self.torch_class([torch.nn.Parameter(torch.zeros(1))], lr=lr, **torch_defaults).param_groups[0])
        for k in _UNSUPPORTED:
            if group.get(k):
                raise ValueError('FusedTorchOptim(%s): %s=%r is not implemented' % (algo, k, group[k]))
        if group.get('fused') or (self.algo != _lib.OPT_ADAMW and group.get('decoupled_weight_decay')):
            raise ValueError('FusedTorchOptim(%s): fused / decoupled_weight_decay are not options of this class' % algo)
        group.pop('params')
        self.arena, self.task = arena, task
        named = list(named_params)
        self.all_params = [p for _, p in named]                     # the order state_dict() indexes by
        self._tb = _Table(arena, {id(p) for _, p in named}, _task_key(task), _lib.OptimTensor)
        self.params = self._tb.params                                           # arena order: the kernel's tensor table
        self._by_id = {id(p): p for p in self.params}
        self.names = {id(p): n for n, p in named if id(p) in self._by_id}
        group['params'] = self.all_params
        self.param_groups = [group]
        dev = arena.flat.device
        self._cuda = dev.type == 'cuda'
        nm = len(_MOMENTS[self.algo])
        self.exp_avg = torch.zeros_like(arena.flat) if nm == 2 else None
        self.exp_avg_sq = torch.zeros_like(arena.flat) if nm >= 1 else None      # (RMSprop's square_avg)
        self._t = torch.zeros(1, dtype=torch.int64, device=dev)                 # completed steps, shared by every covered parameter
        self._norm = torch.zeros(2, dtype=torch.float32, device=dev)            # [squared norm being accumulated, that of the last step]
        self._hyper = _Upload(ctypes.sizeof(_lib.OptimHyper), dev)              # struct goat_optim_hyper: six doubles
        self._hyper_host = None
        self._max_norm = 40.0
        self._table_sig, self._done, self._keep = None, set(), []
        self.last_refreshed = 0
        self._upload_hyper()
        self._build_table()

    # -- the device-resident hyper-parameters ----------------------------------------------------------------------------------------
    def _hyper_values(self):
        g = self.param_groups[0]
        if self.algo in (_lib.OPT_ADAMW, _lib.OPT_ADAM):
            b1, b2 = g['betas']
        else:
            b1, b2 = g.get('alpha', 0.0), 0.0
        mn = self._max_norm
        return (float(g['lr']), float(b1), float(b2), float(g.get('eps', 0.0)), float(g['weight_decay']), float(mn) if mn is not None and mn > 0 else 0.0)

    def _upload_hyper(self):
        """param_groups[0] (and the clip norm) -> the device block, when they changed: pinned and stream-ordered, so a replay launched after
        this call reads the new values and one launched before it the old ones.  Never inside a capture."""
        vals = self._hyper_values()
        if vals == self._hyper_host:
            return
        if self._cuda and torch.cuda.is_current_stream_capturing():
            raise RuntimeError('FusedTorchOptim: hyper-parameters changed inside a hipGraph capture (%r -> %r); call set_lr() / step() with '
                               'these values once before capturing — a captured step reads them from device memory' % (self._hyper_host, vals))
        self._hyper.send(torch.tensor(vals, dtype=torch.float64).view(torch.uint8))
        self._hyper_host = vals

    def set_lr(self, lr):
        """The schedule's step between replays of a captured iteration: lr may be a number or a callable of the current learning rate
        (lr_scheduler-style lambdas take the step; use a closure for that)."""
        g = self.param_groups[0]
        g['lr'] = float(lr(g['lr'])) if callable(lr) else float(lr)
        self._upload_hyper()

    # -- the tensor table: parameters, arena offsets, the cached copies the kernel refreshes itself ---------------------------------
    def _signature(self):
        sig = []
        for p in self.params:
            cache = p.__dict__.get('_goat_shadow')
            if cache:
                sig.append((id(p), tuple((k, t.data_ptr()) for k, (_, t) in cache.items())))
        return tuple(sig)

    def _build_table(self):
        """Once, and again only when the set of cached copies changed (a new operand dtype, a first bf16 pass).  Never inside a capture:
        there the table in use stays, and the copies it does not cover are rebuilt by refresh_shadows (device work, captured)."""
        sig = self._signature()
        if sig == self._table_sig:
            return
        if self._cuda and torch.cuda.is_current_stream_capturing():
            return
        done = self._tb.fill()
        self._tb.send()
        # the table holds raw addresses: the copies it names stay alive as long as it is in use
        self._keep = [t for p in self.params for _, t in (p.__dict__.get('_goat_shadow') or {}).values()]
        self._table_sig, self._done = sig, done

    def step(self, max_norm=40.0):
        """clip_grad_norm_(max_norm) + the update of `algo` on the covered parameters; max_norm None or <= 0: no clipping."""
        from . import hipops
        if not self.params:
            return
        self._max_norm = max_norm
        self._upload_hyper()
        self._build_table()
        arena, tb = self.arena, self._tb
        launch('goat_grad_sqnorm', arena.flat, tb.ranges, tb.n_ranges, self._norm)
        launch('goat_optim_step', self.algo, arena.flat, self.exp_avg, self.exp_avg_sq, tb.dev, tb.chunks, tb.nchunks, self._hyper.dev,
               self._t, self._norm)
        launch('goat_optim_advance', self._t, self._norm, _ptr(self._norm, 1))
        # the copies the kernel did not cover (transposed / float32 images of the parity mode, a third bf16 copy): same storage, new values
        by_id, done = self._by_id, self._done
        self.last_refreshed = sum(hipops.refresh_shadows(p, by_id, done) for p in self.params)

    def last_grad_norm(self):
        """total gradient norm of the last step() (synchronises)."""
        return float(self._norm[1].sqrt().item())

    def steps_done(self):
        """the device counter (synchronises)."""
        return int(self._t.item())

    def _moments_of(self, p):
        a = self.arena.offsets[id(p)]
        bufs = (self.exp_avg, self.exp_avg_sq) if self.algo in (_lib.OPT_ADAMW, _lib.OPT_ADAM) else (self.exp_avg_sq,)
        return {k: b[a:a + p.numel()].view_as(p) for k, b in zip(_MOMENTS[self.algo], bufs)}

    def state_of(self, p):
        """{'step', moments as views into the moment arenas} of a covered parameter (synchronises for the step)."""
        st = {'step': self.steps_done()}
        st.update(self._moments_of(p))
        return st

    # -- torch's optimizer checkpoint format (M/r2r/agent_base.py:205-253 saves / loads optimizer.state_dict()) ----------------------
    def state_dict(self):
        """What torch.optim.<X>(params).state_dict() returns after the same steps: state keyed by the index of the parameter in the
        `named_params` order, entries only for the stepped (covered) parameters, 'step' as the installed torch writes it (a float32
        scalar tensor from 1.12 on, an int before), moments as copies — a view would drag the whole moment arena into torch.save."""
        t = self.steps_done()
        step_as_tensor = tuple(int(x) for x in torch.__version__.split('+')[0].split('.')[:2]) >= (1, 12)
        state = {}
        if t > 0 and self.algo != _lib.OPT_SGD:
            for i, p in enumerate(self.all_params):
                if id(p) in self._by_id:
                    ent = {'step': torch.tensor(float(t), dtype=torch.float32) if step_as_tensor else t}
                    ent.update({k: v.clone() for k, v in self._moments_of(p).items()})
                    state[i] = ent
        group = {k: v for k, v in self.param_groups[0].items() if k != 'params'}
        group['params'] = list(range(len(self.all_params)))
        return {'state': state, 'param_groups': [group]}

    def load_state_dict(self, sd):
        """A checkpoint of torch's optimizer over the same parameter list (or state_dict() of this class).  'step' an int (torch 1.9) or
        a tensor, moments on any device.  Refused: another number of parameters, a moment of another shape, steps that differ among
        the covered parameters (this class keeps ONE counter).  Entries of parameters outside the arena are ignored."""
        groups = sd['param_groups']
        if len(groups) != 1 or len(groups[0]['params']) != len(self.all_params):
            raise ValueError('loaded state dict has %d parameter group(s) / %d parameters, this optimizer one group of %d'
                             % (len(groups), len(groups[0]['params']) if groups else 0, len(self.all_params)))
        state, keys = sd['state'], _MOMENTS[self.algo]
        steps, loads = set(), []
        for i, p in enumerate(self.all_params):
            if id(p) not in self._by_id:
                continue
            ent = state.get(groups[0]['params'][i])
            if not ent or (not keys and 'step' not in ent):
                steps.add(0)
                continue
            stp = ent.get('step', 0)
            steps.add(int(round(float(stp.item() if torch.is_tensor(stp) else stp))))
            for k in keys:
                if k not in ent:
                    raise ValueError('state of parameter %d (%s) has no %r' % (i, self.names[id(p)], k))
                if tuple(ent[k].shape) != tuple(p.shape):
                    raise ValueError('state %r of parameter %d (%s) has shape %s, the parameter %s'
                                     % (k, i, self.names[id(p)], tuple(ent[k].shape), tuple(p.shape)))
                loads.append((p, k, ent[k]))
        if self.algo == _lib.OPT_SGD:
            steps = {0}                       # (torch's SGD without momentum keeps no state)
        if len(steps) > 1:
            raise ValueError('the covered parameters were stepped a different number of times (%s): one counter cannot hold that' % sorted(steps))
        old = self.param_groups[0]
        new = {k: v for k, v in groups[0].items() if k != 'params'}
        for k in _UNSUPPORTED:
            if new.get(k):
                raise ValueError('loaded parameter group has %s=%r: not implemented' % (k, new[k]))
        old.update(new)
        for buf in (self.exp_avg, self.exp_avg_sq):
            if buf is not None:
                buf.zero_()
        for p, k, v in loads:
            self._moments_of(p)[k].copy_(v.detach().to(torch.float32))
        self._t.fill_(steps.pop() if steps else 0)
        self._upload_hyper()


def build_nav_optimizers(args, vln_bert, critic, arena):
    """M/r2r/agent_base.py:107-123 on the arena: (FusedTorchOptim over vln_bert, torch's optimizer of args.optim over the critic's
    parameters), both with lr = args.lr and torch's defaults.  The critic never receives a gradient (train_rl is off upstream), so
    torch's step skips every one of its parameters."""
    if args.optim not in _TORCH_OPTIM:
        raise ValueError('invalid optimizer %r' % (args.optim,))
    opt = FusedTorchOptim(vln_bert.named_parameters(), arena, algo=args.optim, lr=args.lr)
    return opt, getattr(torch.optim, _TORCH_OPTIM[args.optim][0])(critic.parameters(), lr=args.lr)
