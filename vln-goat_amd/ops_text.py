"""Text and feature glue of the back-translation augmentation (inference only; csrc/backtrans.hip): decoded speaker words to the
agent's instruction rows, and the shared environment-dropout mask multiplied into feature columns."""
import torch

from ._plumbing import _dt, _inference_only, launch

RETOK_MAXL = 512            # goat_retok_rows: columns of a row of words, and tokens of an instruction
RETOK_MAXB = 1024
RETOK_STATUS = {1: 'the row has fewer than 2 columns (or more than the words tensor holds): the reference raises on such a row',
                2: 'a word id outside the speaker vocabulary',
                4: 'the whole row is one run of a single word, nothing is kept: the reference raises on such a row'}


def check_retok_status(status):
    """Raise ValueError for the first row of `status` (int32 [B], as goat_retok_rows leaves it) that is not 0.  Reads it back: this
    synchronises."""
    st = status.cpu().tolist()
    for b, s in enumerate(st):
        if s:
            raise ValueError('retok_rows: row %d: %s' % (b, RETOK_STATUS.get(s, 'status %d' % s)))


def retok_rows(words, table, out_ids, out_masks, bos, eos, pad, agent_bos, agent_eos, fill_id=0, max_len=None, width=None, state=None,
               lens=None, status=None, check=True):
    """The agent's `txt_ids` / `txt_masks` rows of decoded speaker words in one launch (goat_retok_rows): per row the reference's
    `shrink` and `decode_sentence` (speaker.shrink_words / decode_words restate them, quirks included), every word expanded through
    `table` (speaker.RetokTable: .V, .first_start, .first_ids, .rest_start, .rest_ids as int32 device tensors),
    ([agent_bos] + ids + [agent_eos])[:max_len], `fill_id` behind it.
    words int64 [B, ldw] contiguous.  width: the columns to read (>= 2), or None to derive it on the device from `state` (a DecodeState:
    as infer_batch_cached cuts its result).  out_ids int64 [B, ldo], out_masks bool [B, ldo], both contiguous and written in place (a raw
    kernel write: memoised masks of out_masks need layers.refresh_masks(only=[...], force=True)); max_len defaults to ldo.
    -> lens int32 [B].  check=True reads the per-row status back (this synchronises) and raises ValueError on a row the reference would
    have raised on; check=False leaves it in `status` (int32 [B]) for check_retok_status.  Inference only."""
    _inference_only('retok_rows', words, out_ids, out_masks)
    if words.dtype != torch.int64 or words.dim() != 2 or not words.is_contiguous():
        raise ValueError('retok_rows: words are a contiguous int64 [B, ldw]')
    B, ldw = words.shape
    if out_ids.dtype != torch.int64 or out_masks.dtype != torch.bool or out_ids.dim() != 2 or out_ids.shape != out_masks.shape \
            or out_ids.shape[0] != B or not out_ids.is_contiguous() or not out_masks.is_contiguous():
        raise ValueError('retok_rows: out_ids int64 / out_masks bool are contiguous [%d, ldo] tensors of one shape' % B)
    ldo = out_ids.shape[1]
    max_len = ldo if max_len is None else int(max_len)
    if width is None:
        if state is None or state.words is not words:
            raise ValueError('retok_rows: without width= the width comes from state=, the DecodeState that owns `words`')
        width, st = 0, (state.ended, state.end_step, state.pos, state.n_live)
    else:
        width, st = int(width), (None, None, None, None)
        if width < 1:
            raise ValueError('retok_rows: width = %d' % width)
    tabs = (table.first_start, table.first_ids, table.rest_start, table.rest_ids)
    V = int(table.V)
    for t in tabs:
        if t.dtype != torch.int32 or t.device != words.device or not t.is_contiguous():
            raise ValueError('retok_rows: the CSR tables are contiguous int32 tensors on %s' % words.device)
    if tabs[0].numel() != V + 1 or tabs[2].numel() != V + 1:
        raise ValueError('retok_rows: a table of V = %d words has V + 1 starts' % V)
    for t in (out_ids, out_masks) + tuple(x for x in st if x is not None):
        if t.device != words.device:
            raise ValueError('retok_rows: every tensor lives on %s' % words.device)
    dev = words.device
    lens = torch.empty(B, dtype=torch.int32, device=dev) if lens is None else lens
    status = torch.empty(B, dtype=torch.int32, device=dev) if status is None else status
    for name, t in (('lens', lens), ('status', status)):
        if t.dtype != torch.int32 or t.numel() != B or t.device != dev or not t.is_contiguous():
            raise ValueError('retok_rows: %s is a contiguous int32 [%d] on %s' % (name, B, dev))
    # (a bool tensor stores one byte per element: the kernel writes 0 / 1 through its data pointer)
    launch('goat_retok_rows', words, ldw, *st, width, B, V, int(bos), int(eos), int(pad), *tabs, int(agent_bos), int(agent_eos), int(fill_id),
           max_len, out_ids, out_masks, ldo, lens, status, what='goat_retok_rows(B=%d,ldw=%d,width=%d,max_len=%d)' % (B, ldw, width, max_len))
    if check:
        check_retok_status(status)
    return lens


def scale_cols(x, noise, out=None):
    """out[..., c] = x[..., c] * noise[c] for c < D = noise.numel() (goat_scale_cols): one float32 multiply rounded once to x's dtype
    (float32 / bfloat16).  x [..., ld] contiguous with ld >= D; the columns behind D are copied (out=None: a new tensor; out=x: in place,
    they are not touched).  noise float32 [D].  Inference only."""
    _inference_only('scale_cols', x, noise, out)
    if noise.dtype != torch.float32 or noise.dim() != 1 or not noise.is_contiguous() or noise.device != x.device:
        raise ValueError('scale_cols: noise is a contiguous float32 [D] on the device of x')
    D, ld = noise.numel(), x.shape[-1] if x.dim() else 0
    if x.dim() < 1 or ld < D or D < 1 or x.numel() == 0 or not x.is_contiguous():
        raise ValueError('scale_cols: x %s is contiguous with at least D = %d columns' % (tuple(x.shape), D))
    if out is None:
        out = torch.empty_like(x)
    elif out.shape != x.shape or out.dtype != x.dtype or out.device != x.device or not out.is_contiguous():
        raise ValueError('scale_cols: out is a contiguous tensor like x')
    launch('goat_scale_cols', _dt(x), x, out, noise, x.numel() // ld, ld, D, what='goat_scale_cols(rows=%d,ld=%d,D=%d)' % (x.numel() // ld, ld, D))
    return out
