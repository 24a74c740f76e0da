"""The text of the navigator kernels (csrc/navstate_core.hpp, csrc/navexpert_core.hpp) compiled as plain C++ and driven on one thread
over host memory: ONE wrapper, its builder, and ONE walk driver that sets guard bands around every buffer the text writes and compares
every step's tables with a host walk of nav_cases.host_walk.  A test file keeps a module fixture that calls build()."""
import ctypes
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import torch

import nav_cases as N

GUARD = 64          # elements in front of and behind every buffer the kernel text writes; nothing may touch them
WRAPPER = r'''
#include <string.h>
#include <vector>
#include "navexpert_core.hpp"
using namespace navstate;
struct NoSync { void operator()() const {} };
#define WORD(x) {#x, H_##x}
static const struct { const char* name; int at; } header_words[] = {%s};
extern "C" {
int cpu_state_ints(int T, int W, int O, int cap) { return Layout(cap, T, W, O).ints; }
int cpu_log_ints(int T, int cap) { return Layout(cap, T, 1).log_ints; }
int cpu_small_ints(int T, int W, int O, int cap) { return Layout(cap, T, W, O).small + HDR; }
int cpu_expert_doubles(int cap, int max_ref) { return expert_doubles(cap, max_ref); }
int cpu_ws_ints(int B, int T, int W, int O) { return Workspace(B, T, W, O).ints; }
int cpu_ws_live_at(int B, int T, int W, int O) { return Workspace(B, T, W, O).live_at; }
int cpu_header_ints() { return HDR; }
int cpu_header_word(const char* name) {          // the value of H_<name>, -1: no such word
  for (const auto& w : header_words)
    if (!strcmp(w.name, name)) return w.at;
  return -1;
}
void cpu_reset(const int64_t* scan_tab, int32_t* si, double* sd, int32_t* log, const int32_t* ep, int B, int T, int W, int O, int cap) {
  Args a = {};
  a.scan_tab = scan_tab; a.si = si; a.sd = sd; a.log = log; a.B = B; a.T = T; a.W = W; a.cap = cap; a.O = O;
  for (int b = 0; b < B; ++b) reset_episode(a, ep, b, 0, 1, NoSync());
}
// ref: null without the label launch of the nDTW expert
void cpu_step(const int64_t* scan_tab, const int64_t* obj_tab, const int64_t* step_tab, const int64_t* ostep_tab, int32_t* si, double* sd,
              int32_t* log, int32_t* ws, const void* act, const double* u, const int32_t* goal, int mode, int t, int B, int T, int Gp, int G,
              int W, int O, int max_end, int A, int cap, int64_t ignoreid, const int32_t* ref, double* xd, int max_ref) {
  Args a = {scan_tab, step_tab, si, sd, log, ws, act, u, mode, t, B, T, Gp, G, W, A, cap, ignoreid, obj_tab, ostep_tab, goal, O, max_end};
  std::vector<int32_t> staged(Layout(cap, T, W, O).small + HDR);        // odd episodes: with the staged copies a kernel keeps in LDS
  for (int b = 0; b < B; ++b) step_episode(a, b, 0, 1, NoSync(), b %% 2 ? staged.data() : nullptr);
  if (t >= T) return;
  int32_t part[1];
  nav_tail(a, part, 0, 1, NoSync());
  const Expert x = {ref, xd, max_ref};
  double row_s[65];
  int32_t ref_s[65];
  if (ref)
    for (int b = 0; b < B; ++b) ndtw_label(a, x, b, 0, 1, NoSync(), b %% 2 ? row_s : nullptr, b %% 2 ? ref_s : nullptr);
}
}
'''


def build(d, csrc=None, source=WRAPPER):
    """compile the wrapper in directory `d` against the headers in `csrc` (default: the package's) -> its ctypes handle.  The header
    words it can be asked for are those navdev.HEADER names: one the enum H_* does not have fails the compilation."""
    from vln_goat_amd import _lib, navdev
    source = source % ', '.join('WORD(%s)' % name.upper() for name in navdev.HEADER)
    src, so = os.path.join(str(d), 'wrapper.cpp'), os.path.join(str(d), 'libnav_cpu.so')
    open(src, 'w').write(source)
    cmd = [os.environ.get('CXX', 'c++'), '-O1', '-std=c++17', '-ffp-contract=off', '-shared', '-fPIC', '-I', csrc or _lib.CSRC, src, '-o', so]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    h = ctypes.CDLL(so)
    vp, i32 = ctypes.c_void_p, ctypes.c_int
    h.cpu_header_word.argtypes = [ctypes.c_char_p]
    h.cpu_reset.argtypes, h.cpu_reset.restype = [vp] * 5 + [i32] * 5, None
    h.cpu_step.argtypes, h.cpu_step.restype = [vp] * 11 + [i32] * 11 + [ctypes.c_int64, vp, vp, i32], None
    return h


def addr(a):
    assert a.flags['C_CONTIGUOUS']
    return a.ctypes.data


def buf():
    """4 KB nobody reads: a non-null pointer for the argument checks of an entry point -> (its owner, the address)"""
    raw = (ctypes.c_char * 4096)()
    return raw, ctypes.addressof(raw) & ~63


class Guarded:
    """an array between two guard bands of a value the kernel text never writes there"""

    def __init__(self, shape, dtype, fill, inside=None):
        n = int(np.prod(shape))
        self.all = np.full(n + 2 * GUARD, fill, dtype)
        self.a = self.all[GUARD:GUARD + n].reshape(shape)
        self.fill = fill
        if inside is not None:
            self.a[...] = inside

    def intact(self):
        f = np.asarray(self.fill, self.all.dtype)
        band = np.concatenate([self.all[:GUARD], self.all[GUARD + self.a.size:]])
        return bool(((band == f) | ((band != band) & (f != f))).all())


def cpu_walk(h, te, scans, eps, w, mode='forced', objects=None, max_end=4, max_ref=None, probs=None, u=None):
    """reset / step / tail of the kernels' text in `mode` beside the host walk `w` (nav_cases.host_walk): 'forced' under w.acts, 'argmax'
    under w.acts / w.scores / w.bests, 'sample' under the probabilities probs[t] [B, G of step t] and the uniforms u [T, B].  objects (an
    ObjectStore): an object walk; max_ref: with the label launch of the nDTW expert.  Every step's tables are compared with w.parts, the
    guard bands of every buffer after every step.
    -> blocks (the read-back blocks), acts and alive (the log), ot (the ObjectTables | None)"""
    from vln_goat_amd import navdev, rollout
    B, T, W, O = len(eps), te.T, te.W, te.O if objects is not None else 0
    tables = rollout.ScanTables(scans, te.sim.features, device=None)
    ot = rollout.ObjectTables(objects, tables, device=None) if O else None
    scan_tab = np.array([addr(tables.host[name]) for name in navdev.SCAN_TABLES], np.int64)
    obj_tab = np.array([addr(ot.host[name]) for name in navdev.OBJECT_TABLES], np.int64) if O else None
    gw = [int(te.gw(t)) for t in range(T)]
    cap = max(gw) - 2
    log_ints = h.cpu_log_ints(T, cap)
    state = {'si': Guarded((B * h.cpu_state_ints(T, W, O, cap),), np.int32, 0x55555555),
             'sd': Guarded((B * (cap * cap + cap),), np.float64, 7.25),
             'log': Guarded((2 * T * B + B * log_ints,), np.int32, 0x55555555),
             'ws': Guarded((navdev.workspace(B, T, W, O)[0],), np.int32, 0x55555555)}
    if O:           # the object bucket adds one best-object record per node, in the part a kernel stages
        assert h.cpu_state_ints(T, W, O, cap) == h.cpu_state_ints(T, W, 0, cap) + cap
        assert h.cpu_small_ints(T, W, O, cap) == h.cpu_small_ints(T, W, 0, cap) + cap
        state['goal'] = Guarded((B, max_end, 2), np.int32, 0x55555555, navdev.object_goals(eps, ot, max_end, te.sim.obj_fallback))
    if max_ref is not None:
        state['xd'] = Guarded((B * h.cpu_expert_doubles(cap, max_ref),), np.float64, np.nan)
    ref = np.zeros((B, (max_ref or 0) + 1), np.int32)
    ep = np.zeros((B, 4), np.int32)
    for i, e in enumerate(eps):
        name = e['scan'].name
        ep[i] = (tables.ids[name], tables.vp(name, e['path'][0]), rollout.GraphSim._snap(e['heading'], 0.0), tables.vp(name, e['path'][-1]))
        if max_ref is not None:
            ref[i, 0] = len(e['path'])
            ref[i, 1:1 + len(e['path'])] = [tables.vp(name, vp) for vp in e['path']]
    forced = np.zeros((T, B), np.int32)
    forced[:len(w.acts)] = np.asarray(w.acts)
    ptr = lambda k: addr(state[k].a) if k in state else None
    h.cpu_reset(addr(scan_tab), ptr('si'), ptr('sd'), ptr('log'), addr(ep), B, T, W, O, cap)
    names = N.TABLES + (N.OBJECT_TABLES if O else ())
    for t in range(T + 1):
        step, step_tab, ostep_tab = {}, None, None
        if t < T:
            for name in names:
                want = w.parts[t]['s%d_%s' % (t, name)].numpy()
                step[name] = Guarded(want.shape, want.dtype, 85, inside=77)
            step_tab = np.array([addr(step[name].a) for name in N.TABLES], np.int64)
            ostep_tab = np.array([addr(step[name].a) for name in N.OBJECT_TABLES], np.int64) if O else None
        act = forced
        if t > 0 and mode == 'argmax':
            act = np.ascontiguousarray(N.back_rows(w, t - 1), np.float32)
        if t > 0 and mode == 'sample':
            act = np.ascontiguousarray(probs[t - 1], np.float32)
            assert act.shape == (B, gw[t - 1])
        h.cpu_step(addr(scan_tab), None if obj_tab is None else addr(obj_tab), None if step_tab is None else addr(step_tab),
                   None if ostep_tab is None else addr(ostep_tab), ptr('si'), ptr('sd'), ptr('log'), ptr('ws'), addr(act),
                   None if u is None else addr(u), ptr('goal'), navdev.MODES[mode], t, B, T, gw[t - 1] if t > 0 else 0, gw[t] if t < T else 0,
                   W, O, max_end if O else 0, N.A, cap, -100, addr(ref) if max_ref is not None else None, ptr('xd'), max_ref or 0)
        if t < T:
            N.compare(t, {'s%d_%s' % (t, name): torch.from_numpy(step[name].a) for name in names}, w.parts[t], names)
        every = dict(state, **step)
        assert all(g.intact() for g in every.values()), (t, [name for name, g in every.items() if not g.intact()])
    log = state['log'].a
    blocks = log[2 * T * B:].reshape(B, log_ints)
    assert not blocks[:, navdev.H['status']].any(), blocks[:, navdev.H['status']:navdev.H['status_t'] + 1]
    return SimpleNamespace(blocks=blocks, acts=log[:T * B].reshape(T, B), alive=log[T * B:2 * T * B].reshape(T, B).astype(bool), ot=ot)
