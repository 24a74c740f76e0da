"""Weight shadows: cached operand copies of the float32 master weights (bf16 casts, K- / row-padded and concatenated images).

A captured hipGraph has their ADDRESSES baked in, so a stale copy is always rebuilt INTO ITS OWN STORAGE, never replaced by a
new tensor: graphs captured before an optimizer step read the updated weights after it (optim.FusedAdamW and optim.FusedTorchOptim refresh most
copies inside their update kernels and the rest through `refresh_shadows`).  torch only: nothing here launches a hand-written kernel.

The copies of a parameter live in `param.__dict__['_goat_shadow']`: {key: (version, tensor)}.  A key names what the copy holds —
this table is the contract between the accessors below, `refresh_shadows`, optim._copies and the tests:

    kind      key                                   owner (holds the cache)    contents
    PLAIN     (dtype, transposed, pad_k)            the weight                 cast [, K zero-padded by pad_k] [, transposed]
    CAT       ('cat', dtype, transposed, ids)       the first member           rows of the members `ids` concatenated, cast [, transposed]
    CATB      ('catb', ids)                         the first member           float32 biases of the members `ids` concatenated
    ROWPAD    ('rowpad', dtype, rows)               the weight                 cast, zero rows appended up to `rows`
    BPAD      ('bpad', n)                           the bias                   float32, zeros appended up to `n`

`ids` is a tuple of id(parameter); the version of a concatenated copy is the tuple of its members' versions.
"""
import torch

ATTR = '_goat_shadow'
PLAIN, CAT, CATB, ROWPAD, BPAD = 'plain', 'cat', 'catb', 'rowpad', 'bpad'


def key_kind(key):
    """kind of a cache key (a PLAIN key starts with a torch.dtype, every other with its kind)."""
    return key[0] if isinstance(key[0], str) else PLAIN


def member_ids(key):
    """ids of the parameters a concatenated copy (CAT / CATB) is made of."""
    return key[-1]


# -- builders: (source, key) -> fresh tensor; source = the owner, or the list of members of a concatenated copy --------------------
def _build_shadow(param, key):
    dtype, transposed, pad_k = key
    with torch.no_grad():
        w = param.detach()
        if pad_k:
            w = torch.nn.functional.pad(w, (0, pad_k))
        if transposed:
            w = w.t()
        return w.to(dtype).contiguous()


def _build_cat(params, key):
    _, dtype, transposed, _ = key
    with torch.no_grad():
        w = torch.cat([p.detach() for p in params], 0)
        if transposed:
            w = w.t()
        return w.to(dtype).contiguous()


def _build_catb(biases, key):
    with torch.no_grad():
        return torch.cat([x.detach().float() for x in biases], 0).contiguous()


def _build_rows_padded(param, key):
    _, dtype, rows = key
    with torch.no_grad():
        w = torch.zeros((rows, param.shape[1]), dtype=dtype, device=param.device)
        w[:param.shape[0]] = param.detach().to(dtype)
        return w


def _build_bias_padded(bias, key):
    with torch.no_grad():
        b = torch.zeros(key[1], dtype=torch.float32, device=bias.device)
        b[:bias.numel()] = bias.detach().float()
        return b


_BUILD = {PLAIN: _build_shadow, CAT: _build_cat, CATB: _build_catb, ROWPAD: _build_rows_padded, BPAD: _build_bias_padded}


# -- the cache -----------------------------------------------------------------------------------------------------------------------
def _store_shadow(cache, key, ver, w):
    ent = cache.get(key)
    if ent is not None and ent[1].shape == w.shape and ent[1].dtype == w.dtype and ent[1].device == w.device:
        ent[1].copy_(w)
        cache[key] = (ver, ent[1])
        return ent[1]
    cache[key] = (ver, w)
    return w


def _cached(owner, key, version, src):
    """The copy `key` in owner's cache; (re)built from `src` by the key's builder — into its own storage when it exists — if it
    is missing, older than `version` or on another device.  The builder comes from _BUILD, as in refresh_shadows: an accessor
    and the refresh cannot disagree on what a key holds."""
    cache = owner.__dict__.setdefault(ATTR, {})
    ent = cache.get(key)
    if ent is not None and ent[0] == version and ent[1].device == owner.device:
        return ent[1]
    return _store_shadow(cache, key, version, _BUILD[key_kind(key)](src, key))


def _shadow(param, dtype, transposed=False, pad_k=0):
    """dtype-cast (and optionally transposed / K-padded) copy of a float32 master weight, cached."""
    return _cached(param, (dtype, transposed, pad_k), param._version, param)


def _shadow_cat(params, dtype, transposed=False):
    """Row-concatenation of several [N_i,K] weights (fused QKV / KV projection), cached on the first."""
    return _cached(params[0], (CAT, dtype, transposed, tuple(id(p) for p in params)), tuple(p._version for p in params), params)


def _cat_bias(biases):
    return _cached(biases[0], (CATB, tuple(id(b) for b in biases)), tuple(b._version for b in biases), biases)


def _bias_padded(bias, n):
    """float32 [n] copy of a bias with zeros behind it (the 64-padded vocabulary of the MLM decoder), cached like _shadow: built
    once, refreshed in place — not a fill + a copy in every step."""
    return _cached(bias, (BPAD, n), bias._version, bias)


def _shadow_rows_padded(param, dtype, rows):
    """[rows, K] copy of a [N, K] weight (N <= rows, extra rows zero), cached like _shadow."""
    return _cached(param, (ROWPAD, dtype, rows), param._version, param)


def refresh_shadows(param, by_id, done=()):
    """Rebuild, in place, every cached copy hanging off `param` whose storage address is not in `done` (the copies an update
    kernel has already refreshed).  For an optimizer that writes the masters through raw pointers (no version bump).
    by_id: {id(parameter): parameter} of every parameter that may be a member of a concatenated copy."""
    cache = param.__dict__.get(ATTR)
    if not cache:
        return 0
    n = 0
    for key, (ver, t) in list(cache.items()):
        if t.data_ptr() in done:
            continue
        k, src = key_kind(key), param
        if k in (CAT, CATB):
            src = [by_id.get(i) for i in member_ids(key)]
            if any(m is None for m in src):
                del cache[key]          # a member is gone: nothing can read this copy any more
                continue
        t.copy_(_BUILD[k](src, key))
        n += 1
    return n
