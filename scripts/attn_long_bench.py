"""GPU-side time of the long-sequence attention entry points (goat_attn_long_fwd / goat_attn_long_bwd, 257-512 keys) beside the
existing ones at their 256-key limit, bf16, nh = 12, B = 48, dropout 0.1 with a key mask: the C ABI called directly (no autograd /
allocator), operands rotated through 4 buffer sets, 10 launches between two HIP events per repetition, warm-up, median of 25
repetitions.  Prints the time per query-key pair at 300 keys relative to 256.
    python scripts/attn_long_bench.py > profiles/long_attention_kernels.txt"""
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import torch                       # noqa: E402
from vln_goat_amd import _lib      # noqa: E402

torch.cuda.set_device(0)
LIB = _lib.lib()
ROT, NH, H, B, P = 4, 12, 768, 48, 0.1
REPS, INNER, WARM = 25, 10, 3


def median_us(fn):
    for _ in range(WARM * INNER):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(INNER):
            fn()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3 / INNER)
    return statistics.median(times)


def run(name, Lq, Lk, self_attn):
    long_path = Lk > 256
    f_fwd, f_bwd = (LIB.goat_attn_long_fwd, LIB.goat_attn_long_bwd) if long_path else (LIB.goat_attn_fwd, LIB.goat_attn_bwd)
    sets = []
    for _ in range(ROT):
        if self_attn:
            qkv = torch.randn(B, Lq, 3 * H, device='cuda').to(torch.bfloat16)
            q, k, v = (qkv, 0, 3 * H, Lq * 3 * H), (qkv, H, 3 * H, Lq * 3 * H), (qkv, 2 * H, 3 * H, Lq * 3 * H)
            dqkv = torch.empty_like(qkv)
            dq, dk, dv = (dqkv, 0, 3 * H, Lq * 3 * H), (dqkv, H, 3 * H, Lq * 3 * H), (dqkv, 2 * H, 3 * H, Lq * 3 * H)
        else:
            qq = torch.randn(B, Lq, H, device='cuda').to(torch.bfloat16)
            kv = torch.randn(B, Lk, 2 * H, device='cuda').to(torch.bfloat16)
            q, k, v = (qq, 0, H, Lq * H), (kv, 0, 2 * H, Lk * 2 * H), (kv, H, 2 * H, Lk * 2 * H)
            dqq, dkv = torch.empty_like(qq), torch.empty_like(kv)
            dq, dk, dv = (dqq, 0, H, Lq * H), (dkv, 0, 2 * H, Lk * 2 * H), (dkv, H, 2 * H, Lk * 2 * H)
        o = torch.empty(B, Lq, H, device='cuda', dtype=torch.bfloat16)
        do = torch.randn(B, Lq, H, device='cuda').to(torch.bfloat16)
        lse = torch.empty(B * NH * Lq, device='cuda')
        km = torch.zeros(B, Lk, device='cuda')
        sets.append((q, k, v, o, do, dq, dk, dv, lse, km))
    ptr = lambda t: t[0].data_ptr() + t[1] * 2
    st = torch.cuda.current_stream().cuda_stream
    i = [0]

    def fwd():
        q, k, v, o, do, dq, dk, dv, lse, km = sets[i[0] % ROT]
        i[0] += 1
        rc = f_fwd(st, 1, ptr(q), q[2], q[3], ptr(k), k[2], k[3], ptr(v), v[2], v[3], o.data_ptr(), H, Lq * H,
                   km.data_ptr(), None, lse.data_ptr(), B, NH, Lq, Lk, 0.125, P, 1, 0, None)
        assert rc == 0, rc

    def bwd():
        q, k, v, o, do, dq, dk, dv, lse, km = sets[i[0] % ROT]
        i[0] += 1
        rc = f_bwd(st, 1, ptr(q), q[2], q[3], ptr(k), k[2], k[3], ptr(v), v[2], v[3], o.data_ptr(), H, Lq * H,
                   do.data_ptr(), H, Lq * H, ptr(dq), dq[2], dq[3], ptr(dk), dk[2], dk[3], ptr(dv), dv[2], dv[3],
                   km.data_ptr(), None, lse.data_ptr(), None, B, NH, Lq, Lk, 0.125, P, 1, 0, None)
        assert rc == 0, rc
    for _ in range(ROT):
        fwd()                      # every set's o / lse exist before the backward is timed
    tf, tb = median_us(fwd), median_us(bwd)
    pairs = B * NH * Lq * Lk
    print('%-18s %-14s Lq=%3d Lk=%3d | fwd %7.1f us (%.3f ps/pair) | bwd %7.1f us (%.3f ps/pair)' % (
        name, 'goat_attn_long' if long_path else 'goat_attn', Lq, Lk, tf, tf * 1e6 / pairs, tb, tb * 1e6 / pairs), flush=True)
    return tf / pairs, tb / pairs


def main():
    print('bf16, B = %d, nh = %d, dropout %.1f, key mask; median of %d repetitions of %d launches (HIP events), %d warm-up repetitions'
          % (B, NH, P, REPS, INNER, WARM))
    r = {}
    for name, Lq, Lk, self_attn in (('self 256', 256, 256, True), ('self 300', 300, 300, True), ('cross 60<-256', 60, 256, False),
                                    ('cross 60<-300', 60, 300, False), ('cross 300<-60', 300, 60, False)):
        r[name] = run(name, Lq, Lk, self_attn)
    print()
    for a, b in (('self 300', 'self 256'), ('cross 60<-300', 'cross 60<-256')):
        print('time per query-key pair, %s / %s: fwd %.2f  bwd %.2f' % (a, b, r[a][0] / r[b][0], r[a][1] / r[b][1]))


if __name__ == '__main__':
    main()
