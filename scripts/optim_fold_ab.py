"""Same-box A/B of csrc/optim.hip against the parent commit's library: bits, kernel time, bench.py legs.  Writes profiles/optim_fold_ab.txt.

    python scripts/optim_fold_ab.py --parent-lib PATH [--parent-tree DIR] [--parts bits,time,bench] [--out profiles/optim_fold_ab.txt]

PATH is libgoat_hip.so built from the parent commit; the tree's own library is the other side.  Both are loaded through ctypes into one
process and driven directly (no optimizer class in between), so the only thing that differs between the sides is the device code.

bits    goat_adamw_step and goat_optim_step (AdamW, Adam, RMSprop, SGD) on identical buffers laid out as the tensor tables of the edge-shape
        set of tests/test_nav_optim_gpu.py (one element, a bias, one chunk exactly, one chunk + 1, a matrix across chunks, an odd tail, a
        K-padded 7-wide matrix, QKV weights and biases in concatenated copies, a view 4 bytes off the 16-byte grid), with every shadow kind:
        one and two bf16 images, a bf16 image 2 bytes off its 8-byte grid, the row-padded image, float32 images, none.  Three consecutive
        steps with fresh gradients; *sq_norm is written by the host (one value that clips, two that do not), so both sides apply the same
        clip coefficient and no atomic sum order enters.  The fine-tuning kernels run under two hyper-parameter sets (weight decay on and
        beta1 = 0.9; weight decay off and beta1 = 0.4: the other branch of lerp).  Parameters, both moments and every shadow buffer are
        compared with torch.equal after every step; a difference is located (tensor, element index mod 4, size in ulp).
time    each library's goat_adamw_step and goat_optim_step(AdamW) alone, between two device events, on a synthetic table of the
        pre-training model's size (208 M elements, a bf16 shadow on every matrix), both libraries on the SAME buffers; parent and head
        alternate, ROUNDS rounds after WARMUP.
        Accepted when the head's median lies within the parent's own min .. max.
bench   (needs --parent-tree: a checkout of the parent commit with its library built)  bench.py --gpus 1 --full --no-roofline
        --no-cpu-baseline with GOAT_BENCH_ONLY_FRESH=1 in both trees: with_optimizer.ms_per_step and
        train_loop.replay_plus_optimizer_ms_per_step.

Every GPU step is a child process under its own `timeout -k 10`; after a step that fails nothing further is started.
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CHUNK = 65536
WARMUP, ROUNDS = 3, 12
# (name, shape, bf16 images, float32 image): '2' = two bf16 images, 'pad' = row-padded + plain, 'off' = second image 2 bytes off the grid
TENSORS = [('s1', (1,), 0, False), ('s3', (3,), 1, False), ('bias', (768,), 1, True), ('chunk', (65536,), 0, False), ('chunk1', (65537,), 1, False),
           ('mat', (96, 768), 2, False), ('odd', (100003,), 'off', False), ('w7', (768, 7), 'pad', False), ('q', (64, 64), 2, False),
           ('k', (64, 64), 1, False), ('v', (64, 64), 1, False), ('bq', (64,), 0, True), ('bk', (64,), 0, True), ('bv', (64,), 0, True),
           ('shifted', (1029,), 1, False)]
KERNELS = [('goat_adamw_step', None), ('goat_optim_step AdamW', 0), ('goat_optim_step Adam', 1), ('goat_optim_step RMSprop', 2),
           ('goat_optim_step SGD', 3)]
HYPERS = [(1e-3, 0.9, 0.999, 1e-8, 0.01), (1e-3, 0.4, 0.98, 1e-8, 0.0)]        # lr, beta1 (RMSprop: alpha), beta2, eps, weight_decay


def _load(path):
    from vln_goat_amd import _lib          # (imports torch first: both libraries then share the HIP runtime torch loaded)
    h = ctypes.CDLL(path)
    for name in ('goat_adamw_step', 'goat_optim_step'):
        fn = getattr(h, name)
        fn.argtypes, fn.restype = _lib.SIGNATURES[name], ctypes.c_int          # (the stream is the first entry)
    return h


def _numel(shape):
    n = 1
    for s in shape:
        n *= s
    return n


class Side:
    """one library's own copy of every buffer the kernels write; the layout (offsets into the buffers) is the same on both sides"""

    def __init__(self, torch, lib, tensors, struct, init):
        from vln_goat_amd import _lib
        self.torch, self.lib = torch, lib
        up4 = lambda x: (x + 3) & ~3
        off = {'p': 0, 'a': 0, 'b0': 0, 'b1': 0, 'f': 0}
        lay = []
        for name, shape, bf, f32 in tensors:
            n = _numel(shape)
            e = {'name': name, 'n': n, 'p': off['p'] + (1 if name == 'shifted' else 0), 'a': off['a'], 's0': None, 's1': None, 'f': None, 'cols': 0, 'ld0': 0}
            off['p'] = up4(e['p'] + n)
            off['a'] = up4(off['a'] + n)
            if bf == 'pad':
                e['s0'], e['cols'], e['ld0'] = off['b0'], shape[1], shape[1] + 1
                off['b0'] = up4(off['b0'] + shape[0] * (shape[1] + 1))
                e['s1'] = off['b1']
                off['b1'] = up4(off['b1'] + n)
            elif bf:
                e['s0'] = off['b0']
                off['b0'] = up4(off['b0'] + n)
                if bf in (2, 'off'):
                    e['s1'] = off['b1'] + (1 if bf == 'off' else 0)
                    off['b1'] = up4(e['s1'] + n)
            if f32:
                e['f'] = off['f']
                off['f'] = up4(off['f'] + n)
            lay.append(e)
        self.lay = lay
        dev = 'cuda'
        self.p = init['p'].clone() if init else torch.zeros(max(4, off['p']), device=dev)
        self.m, self.v = torch.zeros(max(4, off['a']), device=dev), torch.zeros(max(4, off['a']), device=dev)
        self.b0 = torch.zeros(max(4, off['b0']), dtype=torch.bfloat16, device=dev)
        self.b1 = torch.zeros(max(4, off['b1']), dtype=torch.bfloat16, device=dev)
        self.f = torch.zeros(max(4, off['f']), device=dev)
        self.arena_floats = max(4, off['a'])
        host = (struct * len(lay))()
        chunks = []
        for i, e in enumerate(lay):
            t = host[i]
            t.param, t.arena_off, t.numel, t.cols, t.ld0 = self.p.data_ptr() + 4 * e['p'], e['a'], e['n'], e['cols'], e['ld0']
            t.shadow0 = self.b0.data_ptr() + 2 * e['s0'] if e['s0'] is not None else None
            t.shadow1 = self.b1.data_ptr() + 2 * e['s1'] if e['s1'] is not None else None
            t.shadow_f32 = self.f.data_ptr() + 4 * e['f'] if e['f'] is not None else None
            if struct is _lib.AdamwTensor:             # per-tensor scalars: decay on the matrices only, a lagging bias correction on one
                t.step_size, t.decay = 1e-3 * (1.0 + 0.01 * i), 0.0 if len(tensors[i][1]) == 1 else 1e-5
            for first in range(0, e['n'], CHUNK):
                chunks += [i, first]
        nbytes = ctypes.sizeof(host)
        self.table = torch.frombuffer((ctypes.c_uint8 * nbytes).from_address(ctypes.addressof(host)), dtype=torch.uint8).clone().cuda()
        self.chunks, self.nchunks = torch.tensor(chunks, dtype=torch.int32, device=dev), len(chunks) // 2

    def buffers(self):
        return {'param': self.p, 'exp_avg': self.m, 'exp_avg_sq': self.v, 'shadow0': self.b0, 'shadow1': self.b1, 'shadow_f32': self.f}

    def adamw(self, grad, sq, max_norm, lib=None):
        st = (lib or self.lib).goat_adamw_step(self.torch.cuda.current_stream().cuda_stream, grad.data_ptr(), self.m.data_ptr(), self.v.data_ptr(),
                                      self.table.data_ptr(), self.chunks.data_ptr(), self.nchunks, 0.9, 0.98, 1e-6, max_norm, sq.data_ptr())
        assert st == 0, st

    def optim(self, algo, grad, hyper, step, sq, lib=None):
        st = (lib or self.lib).goat_optim_step(self.torch.cuda.current_stream().cuda_stream, algo, grad.data_ptr(), self.m.data_ptr(), self.v.data_ptr(),
                                      self.table.data_ptr(), self.chunks.data_ptr(), self.nchunks, hyper.data_ptr(), step.data_ptr(), sq.data_ptr())
        assert st == 0, st


def _locate(torch, a, b, lay, key):
    """where two buffers differ: per tensor the count, how many at element index = 3 (mod 4), and the largest difference in ulp"""
    out = []
    off_key = {'param': 'p', 'exp_avg': 'a', 'exp_avg_sq': 'a', 'shadow0': 's0', 'shadow1': 's1', 'shadow_f32': 'f'}[key]
    for e in lay:
        o = e[off_key]
        if o is None or (key == 'shadow0' and e['cols']):
            continue
        x, y = a[o:o + e['n']], b[o:o + e['n']]
        ne = (x != y).nonzero().flatten()
        if ne.numel():
            bits = torch.int32 if x.dtype == torch.float32 else torch.int16
            ulp = int((x.view(bits)[ne].long() - y.view(bits)[ne].long()).abs().max())
            out.append('%s: %d of %d elements (%d at index 3 mod 4), up to %d ulp' % (e['name'], ne.numel(), e['n'], int((ne % 4 == 3).sum()), ulp))
    return out


def bits(parent_lib):
    import torch
    from vln_goat_amd import _lib
    libs = {'parent': _load(parent_lib), 'head': _load(_lib.LIB_PATH)}
    gen = torch.Generator().manual_seed(0)
    total = sum(((_numel(s) + 3) & ~3) + 4 for _, s, _, _ in TENSORS)
    init = {'p': (torch.randn(total, generator=gen) * 0.5).cuda()}
    result = {}
    runs = [(label, algo, None) for label, algo in KERNELS[:1]] + [(label, algo, h) for label, algo in KERNELS[1:] for h in HYPERS]
    for label, algo, hyp in runs:
        struct = _lib.AdamwTensor if algo is None else _lib.OptimTensor
        sides = {k: Side(torch, h, TENSORS, struct, init) for k, h in libs.items()}
        step = torch.zeros(1, dtype=torch.int64, device='cuda')
        max_norm = 5.0 if algo is None else 40.0
        hyper = torch.tensor(list(hyp) + [max_norm], dtype=torch.float64).cuda() if hyp else None
        diffs = []
        for it, norm in enumerate((57.25, 3.5, 2.875)):                     # the first clips at 5 and at 40, the others do not
            grad = (torch.randn(sides['head'].arena_floats, generator=gen) * (0.1 if it == 0 else 0.006)).cuda()
            sq = torch.tensor([norm * norm], dtype=torch.float32).cuda()
            for s in sides.values():
                if algo is None:
                    s.adamw(grad, sq, max_norm)
                else:
                    s.optim(algo, grad, hyper, step, sq)
            torch.cuda.synchronize()
            step += 1
            pa, he = sides['parent'].buffers(), sides['head'].buffers()
            for key in pa:
                if not torch.equal(pa[key], he[key]):
                    diffs.append('step %d %s: %s' % (it, key, '; '.join(_locate(torch, pa[key], he[key], sides['head'].lay, key)) or 'row-padded image'))
        assert float(sides['head'].p.abs().sum()) > 0 and not torch.equal(sides['head'].p, init['p'])
        name = label if hyp is None else '%s (beta1 %.1f, weight decay %g)' % (label, hyp[1], hyp[4])
        result[name] = diffs
    print('RESULT ' + json.dumps({'device': torch.cuda.get_device_name(0), 'kernels': result,
                                  'elements': sum(_numel(s) for _, s, _, _ in TENSORS)}))


def time_child(parent_lib):
    import torch
    from vln_goat_amd import _lib
    libs = {'parent': _load(parent_lib), 'head': _load(_lib.LIB_PATH)}
    # 196 matrices of 1024 x 1024 with a bf16 image and 2 560 vectors of 1024: 208.1 M elements
    tensors = [('w%d' % i, (1024, 1024), 1, False) for i in range(196)] + [('b%d' % i, (1024,), 0, False) for i in range(2560)]
    elements = sum(_numel(s) for _, s, _, _ in tensors)
    gen = torch.Generator().manual_seed(1)
    grad = (torch.randn(elements, generator=gen) * 0.01).cuda()
    sq = torch.tensor([4.0], dtype=torch.float32).cuda()
    step = torch.zeros(1, dtype=torch.int64, device='cuda')
    hyper = torch.tensor([1e-5, 0.9, 0.999, 1e-8, 0.01, 40.0], dtype=torch.float64).cuda()
    # ONE set of buffers for both libraries: where a buffer lands in memory moves these HBM-bound kernels by several per cent (a first
    # version with a set per side measured its own allocations: 3 % one way for one kernel, 11 % the other way for the other)
    sa, so = Side(torch, None, tensors, _lib.AdamwTensor, None), Side(torch, None, tensors, _lib.OptimTensor, None)
    calls = {k: {'goat_adamw_step': (lambda h=h: sa.adamw(grad, sq, 5.0, lib=h)), 'goat_optim_step(AdamW)': (lambda h=h: so.optim(0, grad, hyper, step, sq, lib=h))}
             for k, h in libs.items()}
    times = {k: {c: [] for c in calls[k]} for k in calls}
    for r in range(WARMUP + ROUNDS):
        for c in ('goat_adamw_step', 'goat_optim_step(AdamW)'):
            for k in (('parent', 'head') if r % 2 == 0 else ('head', 'parent')):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                calls[k][c]()
                e1.record()
                torch.cuda.synchronize()
                if r >= WARMUP:
                    times[k][c].append(e0.elapsed_time(e1))
    print('RESULT ' + json.dumps({'device': torch.cuda.get_device_name(0), 'elements': elements, 'tensors': len(tensors),
                                  'chunks': sum((_numel(s) + CHUNK - 1) // CHUNK for _, s, _, _ in tensors), 'times': times}))


def _run(cmd, limit, cwd=None, env=None):
    r = subprocess.run(['timeout', '-k', '10', str(limit)] + cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=cwd, env=env)
    return r.returncode, r.stdout


def _child(me, what, parent_lib, limit):
    rc, out = _run(me + ['--child', what, '--parent-lib', parent_lib], limit)
    res = [ln for ln in out.splitlines() if ln.startswith('RESULT ')]
    if rc != 0 or not res:
        print(out[-4000:])
        raise SystemExit('%s step failed (exit status %d): nothing further is run on the GPU' % (what, rc))
    print('%s step done' % what, flush=True)
    return json.loads(res[-1][7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent-lib', required=True, help="libgoat_hip.so built from the parent commit's sources")
    ap.add_argument('--parent-tree', default=None, help='checkout of the parent commit with its library built (bench part)')
    ap.add_argument('--parts', default='bits,time,bench')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'optim_fold_ab.txt'))
    ap.add_argument('--child', choices=['bits', 'time'])
    a = ap.parse_args()
    parent_lib = os.path.abspath(a.parent_lib)
    if a.child:
        return bits(parent_lib) if a.child == 'bits' else time_child(parent_lib)
    parts = a.parts.split(',')
    me = [sys.executable, os.path.abspath(__file__)]
    lines = ['csrc/optim.hip, parent commit against this tree (scripts/optim_fold_ab.py): both libraries in one process, one run on one box', '']
    failed = False
    if 'bits' in parts:
        r = _child(me, 'bits', parent_lib, 300)
        lines += ['bits: identical buffers in the layout of the edge-shape tables (%d elements in %d tensors, every shadow kind), three steps, host-written'
                  % (r['elements'], len(TENSORS)), '*sq_norm (clips, then twice not); parameters, both moments and every shadow compared with torch.equal after each step', '']
        for name, diffs in r['kernels'].items():
            lines.append('  %-62s %s' % (name, 'identical' if not diffs else 'DIFFERS'))
            lines += ['      ' + d for d in diffs]
            failed |= bool(diffs)
        lines += ['', 'device: ' + r['device'], '']
    if 'time' in parts:
        r = _child(me, 'time', parent_lib, 420)
        lines += ['time: one call between two device events, %d tensors, %d elements in %d chunks, a bf16 image on every matrix; both libraries on the same buffers, parent and head'
                  % (r['tensors'], r['elements'], r['chunks']), 'alternating, median of %d rounds after %d warm-ups (min .. max), ms' % (ROUNDS, WARMUP), '']
        for c in r['times']['parent']:
            p, h = r['times']['parent'][c], r['times']['head'][c]
            ok = min(p) <= statistics.median(h) <= max(p)
            lines.append('  %-24s parent %8.3f (%.3f .. %.3f)   head %8.3f (%.3f .. %.3f)   head median %s the parent\'s min .. max'
                         % (c, statistics.median(p), min(p), max(p), statistics.median(h), min(h), max(h), 'within' if ok else 'OUTSIDE'))
            failed |= not ok
        lines.append('')
    if 'bench' in parts:
        if not a.parent_tree:
            raise SystemExit('the bench part needs --parent-tree')
        env = dict(os.environ, GOAT_BENCH_ONLY_FRESH='1')
        env.pop('GOAT_HIP_LIB', None)
        lines += ['bench.py --gpus 1 --full --no-roofline --no-cpu-baseline (GOAT_BENCH_ONLY_FRESH=1), ms per step', '']
        for side, tree in (('parent', os.path.abspath(a.parent_tree)), ('head', ROOT)):
            rc, out = _run([sys.executable, 'bench.py', '--gpus', '1', '--full', '--no-roofline', '--no-cpu-baseline'], 600, cwd=tree, env=env)
            res = [ln for ln in out.splitlines() if ln.startswith('{')]
            if rc != 0 or not res:
                print(out[-4000:])
                raise SystemExit('bench.py (%s) failed (exit status %d): nothing further is run on the GPU' % (side, rc))
            j = json.loads(res[-1])
            lines.append('  %-7s headline %8.3f   with_optimizer %8.3f   train_loop replay_plus_optimizer %8.3f'
                         % (side, j['ms_per_step'], j['with_optimizer']['ms_per_step'], j['train_loop']['replay_plus_optimizer_ms_per_step']))
            print('bench.py (%s) done' % side, flush=True)
        lines.append('')
    text = '\n'.join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, 'w').write(text)
    if failed:
        raise SystemExit(3)


if __name__ == '__main__':
    main()
