"""Where a wave of mel_power_rp_kernel spends its cycles at the C2 shape: by part of the frame loop, by workgroup role, and
for the frames off the fast path -- the wait at the loop top for an edge frame against an ordinary one, the lone 17th turn
against a full one, when the two workgroups of a window end, and -- where the launch carries them -- when the emotion group
workgroups (the first ids of the grid) start and how long one takes.  KM_EMOTION_RIDER=1 in the environment puts the per-window
rider back (role 1 then carries it).  Needs a library built with -DKM_MEL_STAMP
(tools/micro/mel_xchg.sh with EXTRA=-DKM_MEL_STAMP):  KM_LIBRARY=tools/micro/bin/libkm_xchg0.so python tools/micro/mel_stamp.py"""
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from koemorph_amd import _lib, synth           # noqa: E402
from koemorph_amd.engine import Engine         # noqa: E402

PARTS = ["loop top / sample wait", "window + pass 1", "exchange 1 (+ next loads issued)", "pass 2", "exchange 2", "pass 3",
         "partner permutation", "post-processing + power stores", "(frame loop exit)", "barrier before mel stage", "mel stage",
         "barrier after mel stage"]


def main():
    B, L = 256, 136448
    eng = Engine()
    eng.load_state_dict(synth.make_core_params(0, style="init"))
    eng.finalize("cuda:0")
    eng.reserve(B, L)
    audio = torch.from_numpy(synth.make_audio(100, B, L, style="uniform")).cuda()
    emo = torch.from_numpy(synth.normal(200, (B, 256))).cuda()
    state = torch.zeros(B, 52, device="cuda"); out = torch.empty(B, 52, device="cuda")
    eng.forward_audio(audio, emo, state=state, first=True, out=out)
    t0 = time.time()
    while time.time() - t0 < 0.4:                    # steady-state clock
        for _ in range(50):
            eng.forward_audio(audio, emo, state=state, out=out)
        torch.cuda.synchronize()
    lib = _lib.load()
    n = 512 * 8 * 24
    buf = (C.c_ulonglong * n)()
    lib.km_debug_mel_stamps.restype = C.c_int
    rc = lib.km_debug_mel_stamps(buf, n)
    assert rc == 0, rc
    st = np.frombuffer(buf, dtype=np.uint64).reshape(512, 8, 24).astype(np.float64)
    # emotion group workgroups: real-time clock at entry and exit of each (all zero where the rider ran; absent in older libraries)
    grp = np.zeros((0, 2))
    if hasattr(lib, "km_debug_mel_group_stamps"):
        gbuf = (C.c_ulonglong * 256)()
        assert lib.km_debug_mel_group_stamps(gbuf, 256) == 0
        grp = np.frombuffer(gbuf, dtype=np.uint64).reshape(128, 2).astype(np.float64)
        grp = grp[grp[:, 0] > 0]
    role1 = "8 chunks" if len(grp) else "8 chunks + emotion rider"
    total = st[:, :, 12]
    print(f"waves: {st.shape[0] * 8}; cycles per wave (first to last stamp): mean {total.mean():.0f}  min {total.min():.0f}  max {total.max():.0f}")
    for even in (0, 1):
        sel = st[even::2]
        tot = sel[:, :, 12].mean()
        print(f"-- workgroups with blockIdx.x = {even} ({'9 chunks' if even == 0 else role1}): {tot:.0f} cycles per wave")
        for i, name in enumerate(PARTS):
            v = sel[:, :, i].mean()
            print(f"   {name:34s} {v:9.0f} cycles  {100 * v / tot:5.1f} %")
    ent, first, last, rt0, rt1, end = (st[:, :, i] for i in (13, 14, 15, 16, 17, 18))
    # the shader-clock counter is per XCD (not comparable across workgroups); the 100 MHz real-time clock is global
    span_rt = rt1.max() - rt0.min()
    ghz = np.median((end - ent) / np.maximum(rt1 - rt0, 1)) / 10.0
    print(f"kernel span (real-time clock): {span_rt / 100:.2f} us; shader-clock counter runs at {ghz:.3f} GHz")
    if len(grp):
        t0 = min(rt0.min(), grp[:, 0].min())
        dur = grp[:, 1] - grp[:, 0]
        print(f"   emotion groups: {len(grp)} workgroups; start {np.mean(grp[:, 0] - t0) / 100:6.2f} us after the first wave of the launch (max "
              f"{np.max(grp[:, 0] - t0) / 100:.2f}); one takes {dur.mean() / 100:6.2f} us (min {dur.min() / 100:.2f}, max {dur.max() / 100:.2f}); the last ends at "
              f"{np.max(grp[:, 1] - t0) / 100:6.2f} us; first front-end wave {(rt0.min() - t0) / 100:.2f} us after the first group; "
              f"kernel span with the groups {(max(rt1.max(), grp[:, 1].max()) - t0) / 100:.2f} us")
        late = np.sort(rt0.min(axis=1) - rt0.min())[::-1]
        print(f"   front-end workgroups by start: the latest 40 begin {late[:40].mean() / 100:6.2f} us after the first (max {late[0] / 100:.2f}), "
              f"the rest {late[40:].mean() / 100:6.2f} us; {int((late > 100).sum())} start more than 1 us late")
    for role in (0, 1):
        sel = slice(role, None, 2)
        print(f"   role {role}: starts {np.mean(rt0[sel] - rt0.min()) / 100:6.2f} us after the first wave (max {np.max(rt0[sel] - rt0.min()) / 100:.2f}); "
              f"prologue {np.mean(first[sel] - ent[sel]) / ghz / 1e3:6.2f} us; loop {np.mean(last[sel] - first[sel]) / ghz / 1e3:6.2f} us; "
              f"ends {np.mean(rt1[sel] - rt0.min()) / 100:6.2f} us (max {np.max(rt1[sel] - rt0.min()) / 100:.2f}, min {np.min(rt1[sel] - rt0.min()) / 100:.2f})")
    # edge frames (padding / ring wrap) and the partial last turn: slots 19-22 of a wave
    edge_cyc, edge_n, part_cyc, full_cyc = (st[:, :, i] for i in (19, 20, 21, 22))
    n_edge = edge_n.sum()
    ord_cyc = (st[:, :, 0].sum() - edge_cyc.sum()) / max(257 * 256 - n_edge, 1)
    print(f"part 0 (loop top / sample wait): {ord_cyc / ghz / 1e3:6.3f} us per ordinary frame; {edge_cyc.sum() / max(n_edge, 1) / ghz / 1e3:6.3f} us per edge "
          f"frame ({int(n_edge)} edge frames)")
    fr0 = st[0::2, 0, :]
    print(f"   wave 0 of a window's first workgroup (frame 0 at kernel start, and frame 256 where that workgroup takes the last chunk): {np.mean(fr0[:, 19] / np.maximum(fr0[:, 20], 1)) / ghz / 1e3:6.3f} us "
          f"(the other waves' first frames: {np.mean(st[0::2, 1:, 0]) / 16.1 / ghz / 1e3:6.3f} us per frame over the whole loop)")
    had = part_cyc[:, 0] > 0
    print(f"partial last turn (hand-out to last barrier): {int(had.sum())} workgroups, mean {part_cyc[had, 0].mean() / ghz / 1e3 if had.any() else 0:6.3f} us "
          f"(max {part_cyc[had, 0].max() / ghz / 1e3 if had.any() else 0:6.3f}); full turn: mean {full_cyc[:, 0].sum() / (256 * (257 // 16)) / ghz / 1e3:6.3f} us")
    wg_end = rt1.max(axis=1) - rt0.min()
    print(f"the two workgroups of a window end {np.mean(np.abs(wg_end[0::2] - wg_end[1::2])) / 100:5.2f} us apart (mean; max "
          f"{np.max(np.abs(wg_end[0::2] - wg_end[1::2])) / 100:5.2f}); the later one at {np.mean(np.maximum(wg_end[0::2], wg_end[1::2])) / 100:6.2f} us")
    frames = 257 * 256 / (512 * 8)
    print(f"frames per wave: {frames:.2f}")


if __name__ == "__main__":
    main()
