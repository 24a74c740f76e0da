"""Validation of a pre-training run on the device: the reference's `validate` and its `validate_mlm` / `_mrc` / `_sap` / `_cfp`
(P/train_r2r_goat.py:410-583) and `validate_og` (P/train_reverie_goat.py:587-612).

The reference reads 3 to 7 Python numbers back per batch (`.item()`), behind a log_softmax / cross_entropy / argmax / == / sum chain of
ATen launches on [48, ~30] tensors, and sums them in float32 atomics whose order changes from run to run.  Here the model's
`compute_loss=False` outputs go to `goat_val_rows` / `goat_val_cfp` (csrc/valstats.hip: one loss and one hit per row, each logit read
once), `goat_val_reduce` adds their sums into a float64 accumulator on the device in a fixed order, and the host reads that accumulator
ONCE per loader.  Under data parallelism one all_reduce(SUM) of the accumulator replaces the reference's all_gather of Python numbers.

  * `ValStats`      the [n_slots, 3] float64 accumulator (loss sum, hits, counted rows per slot) and its row workspaces.
  * `reduce_stats`  the cross-rank sum of an accumulator (any device: a CPU tensor goes through gloo).
  * `validate_mlm` / `validate_mrc` / `validate_sap` / `validate_og` / `validate_cfp`   the reference's `val_log` dicts.
  * `validate`      the reference's dispatch over {task: loader}; returns the logs instead of writing them to TensorBoard."""
import time

import torch

from .ops_heads import val_cfp, val_reduce, val_rows

CFP_SLOTS = ('g', 'l', 'f')


def reduce_stats(acc):
    """Sum `acc` over the ranks of an initialised torch.distributed group of more than one rank (in place, one all_reduce); a single
    process gets it back untouched.  -> acc"""
    dist = torch.distributed
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        dist.all_reduce(acc, op=dist.ReduceOp.SUM)
    return acc


class ValStats:
    """(loss sum, hits, counted rows) of named slots in one float64 [n_slots, 3] device tensor.

        st = ValStats(('g', 'l', 'f'), device)
        st.add_rows('g', logits, labels=...)      # hard labels (negative: ignored row) — or soft=targets
        st.add_cfp(go, vo, fo, to, temperature)    # fills 'g', 'l', 'f'
        st.read()                                  # {'g': (loss_sum, hits, rows), ...}: THE host read (and the all_reduce)

    Nothing between construction and read() synchronises.  The row workspaces are reused from call to call (launches on one stream
    run in order)."""

    def __init__(self, names, device='cuda'):
        self.names = tuple(names)
        if len(set(self.names)) != len(self.names) or not self.names:
            raise ValueError('ValStats: slot names must be distinct and non-empty: %r' % (self.names,))
        self.device = torch.device(device)
        self.acc = torch.zeros(len(self.names), 3, dtype=torch.float64, device=self.device)
        self._loss = self._hit = None

    def _slot(self, slot):
        return self.acc[self.names.index(slot) if isinstance(slot, str) else slot]

    def _rows_ws(self, n):
        if self._loss is None or self._loss.numel() < n:
            self._loss = torch.empty(n, dtype=torch.float32, device=self.device)
            self._hit = torch.empty(n, dtype=torch.int32, device=self.device)
        return self._loss[:n], self._hit[:n]

    def add_rows(self, slot, logits, labels=None, soft=None):
        """logits [M, N] (any row stride; float32, or cast to it), and exactly one of labels int64 [M] / soft float32 [M, N].
        M == 0 (forward_mlm on a batch without a masked token) launches nothing."""
        if (labels is None) == (soft is None):
            raise ValueError('ValStats.add_rows: exactly one of labels / soft')
        if logits.dim() != 2:
            raise ValueError('ValStats.add_rows: logits must be [M, N], got %s' % (tuple(logits.shape),))
        M = logits.shape[0]
        if M == 0:
            return
        loss, hit = self._rows_ws(M)
        labels = val_rows(logits, loss, hit, labels=labels, soft=soft)
        val_reduce(loss, hit, labels, self._slot(slot))

    def add_cfp(self, go, vo, fo, to, temperature):
        """the three image/text problems of validate_cfp on the pooled vectors -> slots 'g', 'l', 'f'"""
        B = go.shape[0]
        if B == 0:
            return
        loss, hit = self._rows_ws(3 * B)
        val_cfp(go, vo, fo, to, temperature, loss, hit)
        for k, name in enumerate(CFP_SLOTS):
            val_reduce(loss[k * B:(k + 1) * B], hit[k * B:(k + 1) * B], None, self._slot(name))

    def read(self):
        """-> {name: (loss sum, hits, rows)} as Python floats; sums over the ranks first where there are several"""
        host = reduce_stats(self.acc).cpu().tolist()
        return {n: tuple(v) for n, v in zip(self.names, host)}


def _model_device(model):
    return next(model.parameters()).device


def _hard_log(st, name, tot_time, rate_key):
    loss, hits, rows = st[name]
    return {'loss': loss / rows, 'acc': hits / rows, rate_key: rows / tot_time}


def _glf_log(st, tot_time):
    n = st['g'][2]
    return {'gloss': st['g'][0] / n, 'lloss': st['l'][0] / n, 'floss': st['f'][0] / n,
            'gacc': st['g'][1] / n, 'lacc': st['l'][1] / n, 'facc': st['f'][1] / n, 'tok_per_s': n / tot_time}


def _mlm_labels(batch):
    """the labels of the masked tokens in the order of the scores: the index cache forward_mlm left on the batch where there is one (no
    boolean-mask indexing, which synchronises), else the reference's `labels[labels != -1]`"""
    cache = batch.get('_goat_cache') if hasattr(batch, 'get') else None
    if cache is not None and 'mlm_tgt' in cache:
        return cache['mlm_tgt']
    labels = batch['txt_labels']
    return labels[labels != -1]


@torch.no_grad()
def validate_mlm(model, val_loader):
    """P/train_r2r_goat.py:438-464 -> {'loss', 'acc', 'tok_per_s'} over the masked tokens"""
    stats = ValStats(('mlm',), _model_device(model))
    st = time.time()
    for batch in val_loader:
        scores = model(batch, task='mlm', compute_loss=False)
        if scores.shape[0]:
            stats.add_rows('mlm', scores, labels=_mlm_labels(batch))
    res = stats.read()
    return _hard_log(res, 'mlm', time.time() - st, 'tok_per_s')


@torch.no_grad()
def validate_mrc(model, val_loader):
    """P/train_r2r_goat.py:472-497 -> {'loss', 'acc', 'feat_per_s'}: the masked VIEW rows only, as the reference scores them (the object
    rows of a REVERIE batch are returned by the model and not used); n_feat is the number of those rows."""
    stats = ValStats(('mrc',), _model_device(model))
    st = time.time()
    for batch in val_loader:
        view_logits, view_targets, _, _ = model(batch, task='mrc', compute_loss=False)
        stats.add_rows('mrc', view_logits, soft=view_targets)
    res = stats.read()
    return _hard_log(res, 'mrc', time.time() - st, 'feat_per_s')


@torch.no_grad()
def validate_sap(model, val_loader):
    """P/train_r2r_goat.py:499-531 -> gloss lloss floss gacc lacc facc tok_per_s; the fused row is scored against the GLOBAL labels"""
    stats = ValStats(CFP_SLOTS, _model_device(model))
    st = time.time()
    for batch in val_loader:
        gl, ll, fl, ga, la = model(batch, task='sap', compute_loss=False)
        stats.add_rows('g', gl, labels=ga)
        stats.add_rows('l', ll, labels=la)
        stats.add_rows('f', fl, labels=ga)
    res = stats.read()
    return _glf_log(res, time.time() - st)


@torch.no_grad()
def validate_og(model, val_loader):
    """P/train_reverie_goat.py:587-612 -> {'loss', 'acc', 'tok_per_s'}"""
    stats = ValStats(('og',), _model_device(model))
    st = time.time()
    for batch in val_loader:
        scores = model(batch, task='og', compute_loss=False)
        stats.add_rows('og', scores, labels=batch['obj_labels'])
    res = stats.read()
    return _hard_log(res, 'og', time.time() - st, 'tok_per_s')


@torch.no_grad()
def validate_cfp(model, val_loader, temperature):
    """P/train_r2r_goat.py:533-583 -> gloss lloss floss gacc lacc facc tok_per_s (candidates: the batch's own vectors, as there)"""
    stats = ValStats(CFP_SLOTS, _model_device(model))
    st = time.time()
    for batch in val_loader:
        go, vo, fo, to = model(batch, task='cfp', compute_loss=False)
        stats.add_cfp(go, vo, fo, to, temperature)
    res = stats.read()
    return _glf_log(res, time.time() - st)


def validate(model, val_dataloaders, setname='', max_metrix=None, tem=None):
    """The reference's `validate` (P/train_r2r_goat.py:410-435; `og` as P/train_reverie_goat.py dispatches it) over {task: loader}:
    eval mode, one validate_* per task by `task.startswith(...)`, then the model's training flag back to what it was (the reference
    calls model.train() whatever it found).  -> (logs, max_metrix, max_update_flag): logs = {'val{setname}_{task}_{k}': value};
    on setname == '_unseen' with a max_metrix given, a sap `facc` >= max_metrix replaces it and raises the flag (:421-424).  An unknown
    task raises ValueError.  Writing the logs to TensorBoard stays with the caller."""
    was_training = model.training
    model.eval()
    logs, max_update_flag = {}, False
    try:
        for task, loader in val_dataloaders.items():
            if task.startswith('mlm'):
                val_log = validate_mlm(model, loader)
            elif task.startswith('mrc'):
                val_log = validate_mrc(model, loader)
            elif task.startswith('sap'):
                val_log = validate_sap(model, loader)
                if setname == '_unseen' and max_metrix is not None and val_log['facc'] >= max_metrix:
                    max_metrix = val_log['facc']
                    max_update_flag = True
            elif task.startswith('og'):
                val_log = validate_og(model, loader)
            elif task.startswith('cfp'):
                val_log = validate_cfp(model, loader, tem)
            else:
                raise ValueError('Undefined task %s' % task)
            logs.update({'val%s_%s_%s' % (setname, task, k): v for k, v in val_log.items()})
    finally:
        model.train(was_training)
    return logs, max_metrix, max_update_flag
