"""The back-door (BACL) dictionary pipeline on the device: the instruction dictionaries the fine-tuning run rebuilds with
--z_instr_update, and the room-type image dictionary.

Reference: M/r2r/agent.py:713-848 (update_z_dict: the encoder pass over the training set, one picked token row per landmark / direction
word, np.mean per key, count / total as p(z)), :850-871 (save_backdoor_z_dict), M/r2r/main_nav.py:190-192,311-322 (where the run calls
them), M/reverie/agent_obj_goat.py:36-138 (the landmark-only form), M/do_utils/do_intervention.py:109-148 (room-type means of the view
features).

What differs from the reference:
  - the hidden states never leave the device: every encoder batch is added into running per-key sums by goat_dict_accumulate
    (csrc/zdict.hip; compensated float32, bitwise reproducible) and one goat_dict_finish per kind writes the means and p(z);
  - the word alignment is done ONCE, on the host, by InstrPickPlan (the reference caches the word picker's lists per instruction and
    repeats the token walk in every update); the spaCy word picker itself stays outside: the caller hands in its lists;
  - the dictionaries live in persistent tensors that an update rewrites in place, the [B, K, H] buffers extras() handed out included,
    so an episode graph captured over them sees the new dictionaries on its next replay;
  - the landmark-only form (kinds=('landmark',)) refreshes p(z) together with the features.  The REVERIE agent keeps the p(z) of the
    dictionary it was given and replaces the features only, which cannot fit once the number of keys changes.
"""
import csv
import sys

import numpy as np
import torch

from . import features, hipops

KINDS = ('direction', 'landmark')
IMG_PICKS_PER_LAUNCH = 65536


# ----------------------------------------------------------------------------- the token walk
def pick_positions(tokens, landmarks, directions):
    """Which rows of an instruction's hidden states feed the dictionaries (the walk of M/r2r/agent.py:778-799).  tokens: the word
    pieces without special tokens; landmarks / directions: the word picker's [(word_index, key), ...] in ascending word order.  Words
    are counted over the tokens that do not start with '#' (a continuation piece belongs to the word before it); when the count
    reaches the word index of the next unused entry of a list, the token is picked for that entry's key — a landmark and a direction
    may both take one token.  -> [(pos, kind, key)] with pos = token index + 1 (row 0 is [CLS]), landmark before direction on a shared
    token.  Entries whose word index is never reached (beyond the tokens, or behind an entry that was not reached) pick nothing."""
    picks = []
    word, li, di = 0, 0, 0
    for j, tok in enumerate(tokens):
        if tok[0] == '#':
            continue
        if li < len(landmarks) and landmarks[li][0] == word:
            picks.append((j + 1, 'landmark', landmarks[li][1]))
            li += 1
        if di < len(directions) and directions[di][0] == word:
            picks.append((j + 1, 'direction', directions[di][1]))
            di += 1
        word += 1
    return picks


class _PlanBatch:
    """One encoder batch of an InstrPickPlan: ids int64 [b, Lmax], mask bool [b, Lmax], and `picks`, ONE int32 tensor that holds, per
    kind with picks in this batch, the rows (b * Lmax + pos, grouped by slot) followed by the start array [K + 1];
    layout[kind] = (offset of rows, number of rows, offset of start).  max_rows[kind]: the most rows one slot has in this batch."""

    def __init__(self, ids, mask, picks, layout, max_rows):
        self.ids, self.mask, self.picks, self.layout, self.max_rows = ids, mask, picks, layout, max_rows
        self.size = ids.shape[0]

    def rows(self, kind, picks=None):
        off, n, _ = self.layout[kind]
        return (self.picks if picks is None else picks)[off:off + n]

    def start(self, kind, K, picks=None):
        _, _, off = self.layout[kind]
        return (self.picks if picks is None else picks)[off:off + K + 1]


class InstrPickPlan:
    """The host half of update_z_dict, built once and used by every update (the reference's instr_specific_dict cache, extended to
    the token walk).  instr_data: the training items, each with 'instr_encoding' (ids with [CLS] ... [SEP]); tokens_of(item) -> the
    tokens of convert_ids_to_tokens(item['instr_encoding'], skip_special_tokens=True); words_of(item) -> (landmarks, directions) of the
    word picker.  Batches of `batch_size` in order, each padded to its longest instruction (M/r2r/agent.py:748-755); max_len cuts longer
    encodings first.  Slots are numbered per kind in the order the keys first appear over the whole pass.

    keys[kind]: the keys in slot order; counts[kind]: {key: picks}; pz[kind]: {key: count / total} (Python floats, :801-812);
    batches: the _PlanBatch list.  A pick at or beyond the instruction's length raises ValueError."""

    def __init__(self, instr_data, tokens_of, words_of, batch_size=64, max_len=None, kinds=KINDS):
        self.batch_size, self.kinds = int(batch_size), tuple(kinds)
        if self.batch_size < 1:
            raise ValueError('InstrPickPlan: batch_size = %d' % batch_size)
        slot = {k: {} for k in KINDS}
        self.counts = {k: {} for k in KINDS}
        raw = []
        for i0 in range(0, len(instr_data), self.batch_size):
            items = instr_data[i0:i0 + self.batch_size]
            encs = [list(it['instr_encoding'])[:max_len] for it in items]
            Lmax = max(len(e) for e in encs)
            ids = np.zeros((len(encs), Lmax), dtype=np.int64)
            mask = np.zeros((len(encs), Lmax), dtype=bool)
            per_kind = {k: [] for k in KINDS}
            for b, (it, enc) in enumerate(zip(items, encs)):
                ids[b, :len(enc)] = enc
                mask[b, :len(enc)] = True
                landmarks, directions = words_of(it)
                for pos, kind, key in pick_positions(tokens_of(it), landmarks, directions if 'direction' in self.kinds else []):
                    if kind not in self.kinds:
                        continue
                    if pos >= len(enc):
                        raise ValueError('InstrPickPlan: item %d picks token row %d for %s %r, its encoding has %d'
                                         % (i0 + b, pos, kind, key, len(enc)))
                    s = slot[kind].setdefault(key, len(slot[kind]))
                    self.counts[kind][key] = self.counts[kind].get(key, 0) + 1
                    per_kind[kind].append((s, b * Lmax + pos))
            raw.append((ids, mask, per_kind))
        self.keys = {k: list(slot[k]) for k in KINDS}
        self.pz = {}
        for k in KINDS:
            total = sum(self.counts[k].values())
            self.pz[k] = {key: n / total for key, n in self.counts[k].items()}
        self.batches = []
        for ids, mask, per_kind in raw:
            parts, layout, max_rows, off = [], {}, {}, 0
            for k in self.kinds:
                K = len(self.keys[k])
                if not per_kind[k]:
                    continue
                per_kind[k].sort(key=lambda sr: sr[0])             # stable: inside a slot the rows keep the order of the walk
                per_slot = np.bincount([s for s, _ in per_kind[k]], minlength=K)
                start = np.zeros(K + 1, dtype=np.int32)
                start[1:] = np.cumsum(per_slot)
                rows = np.array([r for _, r in per_kind[k]], dtype=np.int32)
                layout[k] = (off, len(rows), off + len(rows))
                max_rows[k] = int(per_slot.max())
                off += len(rows) + K + 1
                parts += [rows, start]
            picks = torch.from_numpy(np.concatenate(parts)) if parts else torch.zeros(0, dtype=torch.int32)
            self.batches.append(_PlanBatch(torch.from_numpy(ids), torch.from_numpy(mask), picks, layout, max_rows))
        self._pinned = False

    def pin(self):
        """Page-lock the batch tensors (once), so that every update uploads them with one asynchronous copy each."""
        if not self._pinned and torch.cuda.is_available():
            for b in self.batches:
                b.ids, b.mask, b.picks = b.ids.pin_memory(), b.mask.pin_memory(), b.picks.pin_memory()
            self._pinned = True
        return self


# ----------------------------------------------------------------------------- the instruction dictionaries
def _read_zdict_tokens(path):
    csv.field_size_limit(sys.maxsize)
    names = {k: [] for k in KINDS}
    with open(path, 'rt') as f:
        for item in csv.DictReader(f, delimiter='\t', fieldnames=features.TXT_ZDICT_FIELDS):
            if item['token_type'] in names:
                names[item['token_type']].append(item['token'])
    return names


class InstrDictionaries:
    """The direction / landmark dictionaries of BACL-txt as persistent device tensors, and update_z_dict over them.

    feats[kind] float32 [K, H] and pzs[kind] float32 [K] are the masters; keys[kind] the token names in row order; host_pz[kind]
    {key: float} what the reference computes on the host (it goes to the TSV).  load_tsv() fills them from a dictionary file, update()
    from the model.  kinds=('landmark',) is the REVERIE agent: the encoder is run without dictionaries (as that agent does), only the
    landmark entries exist, and — unlike the reference — their p(z) is refreshed together with the features."""

    def __init__(self, device, H=768, kinds=KINDS):
        self.device, self.H = torch.device(device), int(H)
        self.kinds = tuple(kinds)
        if not self.kinds or any(k not in KINDS for k in self.kinds):
            raise ValueError('InstrDictionaries: kinds are taken from %s, got %s' % (KINDS, kinds))
        self.feats, self.pzs, self.keys, self.host_pz = {}, {}, {}, {}
        self._state = {}
        self._extras = {}             # (B, dtype) -> {kind: ([B, K, H], [B, K, 1])}

    def _k(self, kind):
        return self.feats[kind].shape[0] if kind in self.feats else None

    def _check_k(self, what, new_k):
        """Buffers that were handed out cannot change shape (a captured graph holds them)."""
        if not self._extras:
            return
        for kind in self.kinds:
            if self._k(kind) != new_k[kind]:
                raise ValueError('%s: %d %s keys, but extras() handed out buffers for %d: a captured graph cannot change shape'
                                 % (what, new_k[kind], kind, self._k(kind)))

    def _resize(self, new_k):
        for kind in self.kinds:
            K = new_k[kind]
            if K < 1:
                raise ValueError('InstrDictionaries: no %s keys' % kind)
            if self._k(kind) != K:
                self.feats[kind] = torch.zeros(K, self.H, dtype=torch.float32, device=self.device)
                self.pzs[kind] = torch.zeros(K, dtype=torch.float32, device=self.device)

    def load_tsv(self, path):
        """Read a dictionary file (features.load_instr_zdict; the token names are kept for save_tsv)."""
        z = features.load_instr_zdict(path)
        names = _read_zdict_tokens(path)
        self._check_k('InstrDictionaries.load_tsv', {k: len(names[k]) for k in self.kinds})
        self._resize({k: len(names[k]) for k in self.kinds})
        for kind in self.kinds:
            f, p = z['instr_%s_features' % kind], z['instr_%s_pzs' % kind]
            if f.dim() != 2 or f.shape[1] != self.H:
                raise ValueError('InstrDictionaries.load_tsv: %s features are %s, H = %d' % (kind, tuple(f.shape), self.H))
            self.feats[kind].copy_(f)
            self.pzs[kind].copy_(p)
            self.keys[kind] = names[kind]
            self.host_pz[kind] = dict(zip(names[kind], p.tolist()))
        for bufs in self._extras.values():
            for kind, (bf, bp) in bufs.items():
                bf.copy_(self.feats[kind].unsqueeze(0).expand_as(bf))
                bp.copy_(self.pzs[kind].view(1, -1, 1).expand_as(bp))
        return self

    def z_dict(self):
        """{'instr_zdict': {...}} in the reference's shapes ([K, H] features, [K] p(z)); the tensors are the persistent masters."""
        d = {}
        for kind in self.kinds:
            d['instr_%s_features' % kind] = self.feats[kind]
            d['instr_%s_pzs' % kind] = self.pzs[kind]
        return {'instr_zdict': d}

    def update(self, model, plan):
        """update_z_dict (M/r2r/agent.py:713-848): the model in eval mode, mode='instr_zdict_update' under no_grad for every batch of
        `plan` with the CURRENT dictionaries as inputs (None before any exist), the picked rows of every output added on the device;
        the dictionaries are rewritten once, after the last batch, so every batch of one update reads the old ones.  The model's
        training flag is put back.  -> (z_dict, landmark features by token, direction features by token, landmark p(z) by token,
        direction p(z) by token): the feature values are rows of the persistent device masters, the p(z) Python floats.  A kind this
        object does not hold gives empty dicts."""
        new_k = {k: len(plan.keys[k]) for k in self.kinds}
        for kind in self.kinds:
            if new_k[kind] < 1:
                raise ValueError('InstrDictionaries.update: the plan has no %s picks' % kind)
        self._check_k('InstrDictionaries.update', new_k)
        plan.pin()
        feed = {'instr_z_direction_features': None, 'instr_z_direction_pzs': None, 'instr_z_landmark_features': None,
                'instr_z_landmark_pzs': None}
        if set(self.kinds) == set(KINDS) and all(k in self.keys for k in KINDS):      # (one kind alone: no inputs, as the REVERIE agent)
            for kind in KINDS:
                feed['instr_z_%s_features' % kind] = self.feats[kind].unsqueeze(0).repeat(plan.batch_size, 1, 1)
                feed['instr_z_%s_pzs' % kind] = self.pzs[kind].view(1, -1, 1).repeat(plan.batch_size, 1, 1)
        states = {}
        for kind in self.kinds:
            st = self._state.get(kind)
            if st is None or st.K != new_k[kind]:
                st = self._state[kind] = hipops.DictState(new_k[kind], self.H, self.device)
            states[kind] = st.zero()
        was_training = model.training
        model.eval()
        try:
            with torch.no_grad():
                for batch in plan.batches:
                    ids = batch.ids.to(self.device, non_blocking=True)
                    mask = batch.mask.to(self.device, non_blocking=True)
                    picks = batch.picks.to(self.device, non_blocking=True)
                    inputs = {'z_txt': ids, 'z_txt_mask': mask, 'front_txt_feats': None}
                    for name, t in feed.items():
                        inputs[name] = None if t is None else t[:batch.size]
                    out = model('instr_zdict_update', inputs).detach()
                    if out.dim() != 3 or tuple(out.shape[:2]) != tuple(ids.shape) or out.shape[2] != self.H:
                        raise ValueError('InstrDictionaries.update: the model returned %s for ids %s, H = %d'
                                         % (tuple(out.shape), tuple(ids.shape), self.H))
                    x = out.contiguous().view(-1, self.H)
                    for kind in self.kinds:
                        if kind in batch.layout:
                            hipops.dict_accumulate(x, batch.rows(kind, picks), batch.start(kind, new_k[kind], picks), states[kind])
                self._resize(new_k)
                for kind in self.kinds:
                    hipops.dict_finish(states[kind], feats=self.feats[kind], out_pz=self.pzs[kind].view(1, -1))
                    for bufs in self._extras.values():
                        hipops.dict_finish(states[kind], out=bufs[kind][0], out_pz=bufs[kind][1])
                    self.keys[kind] = list(plan.keys[kind])
                    self.host_pz[kind] = dict(plan.pz[kind])
        finally:
            model.train(was_training)
        by_token = {k: ({key: self.feats[k][i] for i, key in enumerate(self.keys[k])} if k in self.kinds else {}) for k in KINDS}
        pz = {k: (dict(self.host_pz[k]) if k in self.kinds else {}) for k in KINDS}
        return self.z_dict(), by_token['landmark'], by_token['direction'], pz['landmark'], pz['direction']

    def extras(self, B, dtype=None):
        """The 'language' dictionary entries of synth.rollout_extras: instr_z_<kind>_features [B, K, H] and instr_z_<kind>_pzs
        [B, K, 1] of `dtype` (default float32) holding the current dictionaries.  One set of buffers per (B, dtype), handed out again on
        every call and rewritten in place by every later update() / load_tsv()."""
        dtype = dtype or torch.float32
        key = (int(B), dtype)
        if key not in self._extras:
            if any(k not in self.keys for k in self.kinds):
                raise ValueError('InstrDictionaries.extras: no dictionaries yet (load_tsv or update first)')
            self._extras[key] = {k: (self.feats[k].to(dtype).unsqueeze(0).repeat(key[0], 1, 1),
                                     self.pzs[k].to(dtype).view(1, -1, 1).repeat(key[0], 1, 1)) for k in self.kinds}
        lang = {}
        for kind, (bf, bp) in self._extras[key].items():
            lang['instr_z_%s_features' % kind] = bf
            lang['instr_z_%s_pzs' % kind] = bp
        return {'language': lang}

    def save_tsv(self, path):
        """The file of save_backdoor_z_dict (M/r2r/agent.py:850-871; backdoor_update_features.tsv): landmarks first, then directions,
        one line `token_type <tab> token <tab> base64(float32 feature) <tab> pz`; features.load_instr_zdict reads it."""
        rows = []
        for kind in ('landmark', 'direction'):
            if kind not in self.kinds:
                continue
            f = self.feats[kind].detach().float().cpu().numpy()
            for i, key in enumerate(self.keys[kind]):
                rows.append({'token_type': kind, 'token': key, 'feature': f[i], 'pz': self.host_pz[kind][key]})
        features.write_zdict_tsv(path, rows, features.TXT_ZDICT_FIELDS)


# ----------------------------------------------------------------------------- the image dictionary
def img_zdict_keys(roomtypes, roomnum=50):
    """The host half of build_zdict_and_pz (M/do_utils/do_intervention.py:109-148).  roomtypes: {'<scan>_<vp>': [label per view]}.
    The `roomnum` most frequent labels are kept — a stable descending sort of the labels in first-appearance order, so of equally
    frequent labels the one seen first stays; the dictionary rows are in the order the kept labels first appear.
    -> (labels in row order, {label: count}, {label: count / kept total})."""
    totals = {}
    for labels in roomtypes.values():
        for lab in labels:
            totals[lab] = totals.get(lab, 0) + 1
    kept = sorted(totals.items(), key=lambda kv: kv[1], reverse=True)[:roomnum]
    kept_total = sum(n for _, n in kept)
    keep = dict(kept)
    order = [lab for lab in totals if lab in keep]       # dicts keep insertion order: first appearance over the iteration
    return order, {lab: keep[lab] for lab in order}, {lab: keep[lab] / kept_total for lab in order}


def build_img_zdict(store, roomtypes, roomnum=50):
    """The room-type image dictionary: per kept label the mean of the view features that carry it, and p(z) (the reference:
    M/do_utils/do_intervention.py:109-148, np.mean over lists of rows).  store: a FeatureStore resident on the device (.to(device));
    roomtypes: {'<scan>_<vp>': [label of view 0 .. view 35]}.  The means are taken on the device by goat_dict_accumulate over
    store.dev, at most IMG_PICKS_PER_LAUNCH picked rows per launch.
    -> {'img_features': float32 [K, D] on the device, 'img_pzs': float64 [K], 'roomtypes': the labels in row order}."""
    if store.dev is None:
        raise RuntimeError('build_img_zdict: the store is not on the device (call .to(device) first)')
    order, counts, pz = img_zdict_keys(roomtypes, roomnum)
    if not order:
        raise ValueError('build_img_zdict: no labels')
    slot = {lab: i for i, lab in enumerate(order)}
    K, D = len(order), store.dev.shape[1]
    per_slot = [[] for _ in order]
    for key, labels in roomtypes.items():
        if key not in store.index:
            raise KeyError('build_img_zdict: %r is not in the feature store' % key)
        if len(labels) > store.views:
            raise ValueError('build_img_zdict: %r has %d labels for %d views' % (key, len(labels), store.views))
        base = store.index[key] * store.views
        for view, lab in enumerate(labels):
            if lab in slot:
                per_slot[slot[lab]].append(base + view)
    slots = np.repeat(np.arange(K), [len(r) for r in per_slot])
    rows = np.concatenate([np.asarray(r, dtype=np.int32) for r in per_slot])
    state = hipops.DictState(K, D, store.dev.device)
    with torch.no_grad():
        for p0 in range(0, len(rows), IMG_PICKS_PER_LAUNCH):
            sl = slots[p0:p0 + IMG_PICKS_PER_LAUNCH]
            start = np.zeros(K + 1, dtype=np.int32)
            start[1:] = np.cumsum(np.bincount(sl, minlength=K))
            packed = torch.from_numpy(np.concatenate([rows[p0:p0 + IMG_PICKS_PER_LAUNCH], start]))
            if store.dev.is_cuda:
                packed = packed.pin_memory()
            packed = packed.to(store.dev.device, non_blocking=True)
            hipops.dict_accumulate(store.dev, packed[:len(sl)], packed[len(sl):], state)
        feats = torch.empty(K, D, dtype=torch.float32, device=store.dev.device)
        hipops.dict_finish(state, feats=feats)
    return {'img_features': feats, 'img_pzs': torch.tensor([pz[lab] for lab in order], dtype=torch.float64), 'roomtypes': order}


def write_img_zdict(path, zdict):
    """Write what build_img_zdict returned as the reference's image_z_dict file (`roomtype <tab> base64(float32 feature) <tab> pz`);
    features.load_img_zdict reads it."""
    f = zdict['img_features'].detach().float().cpu().numpy()
    rows = [{'roomtype': lab, 'feature': f[i], 'pz': float(zdict['img_pzs'][i])} for i, lab in enumerate(zdict['roomtypes'])]
    features.write_zdict_tsv(path, rows, features.IMG_ZDICT_FIELDS)
