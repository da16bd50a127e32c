"""Workgroup stamps of step_end_kernel (profiles/r06_step_end_stamps.log, r07_step_end_tail_stamps.log).

Needs a library built with the stamps (make -C sxmc_amd/csrc VARIANT=_stamps EXTRA=-DSXMC_WG_STAMPS=1) named by
SXMC_HIP_LIB.  Config 3's step end at its full row count (tables at 1/50 of their size, which the step end does not
see): 300 steps launched one by one after 50, each read back after its step.  A worker stamps its entry, its first row's
gathers having landed and its slot stored; the finisher its entry, all partials held, and its exit (100 MHz counter).

  SXMC_HIP_LIB=.../libsxmc_hip_stamps.so python tools/step_end_stamps.py [workers]

`workers`: workgroups of the event sum (rows / 128, rounded up; 51 at this set-up) -- the finisher is the one after them.
"""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from sxmc_amd import capi, workloads  # noqa: E402
from sxmc_amd.mcmc import MCMC  # noqa: E402


def main():
    nw = int(sys.argv[1]) if len(sys.argv) > 1 else 51
    w = workloads.config3(0.02, nevents=100000)
    m = MCMC(w, seed=3, lut_output=False, consume=True, stream=capi.new_stream())
    m.setup(w.events, sync_interval=400)
    lib = capi.load()
    if not hasattr(lib, "sxmc_debug_read_wg_stamps"):
        raise SystemExit("SXMC_HIP_LIB must name a library built with -DSXMC_WG_STAMPS=1")
    lib.sxmc_debug_read_wg_stamps.argtypes = [C.c_void_p, C.c_int]
    lib.sxmc_debug_read_wg_stamps.restype = C.c_int
    buf = np.zeros(3 * 4096, np.uint64)
    for _ in range(50):
        m.step()
    capi.synchronize()
    steps = []
    for _ in range(300):
        m.step()
        capi.synchronize()
        if lib.sxmc_debug_read_wg_stamps(buf.ctypes.data_as(C.c_void_p), buf.size) != 0:
            raise SystemExit("reading the stamps failed")
        # (the step end runs after the fill and stamps over its first workgroups' entries: 0 .. nw)
        steps.append(buf.reshape(3, 4096)[:, : nw + 1].astype(np.int64))
    print("launches per step %d, step_end_timeouts %d" % (m.group.LastStepLaunches(), m.group.StepEndTimeouts()))
    a = np.array(steps, np.float64) * 0.01                   # us
    t0 = a[:, 0, :].min(axis=1)                              # the first workgroup's entry

    def line(name, v):
        print("%-30s %6.2f [%6.2f, %6.2f]" % (name, np.median(v), np.percentile(v, 10), np.percentile(v, 90)))

    print("steps %d, workers %d; us after the first workgroup's entry: median over steps [p10, p90]" % (a.shape[0], nw))
    entry, landed, stored = (a[:, k, :nw] - t0[:, None] for k in range(3))
    line("worker entry med", np.median(entry, axis=1))
    line("worker entry max", entry.max(axis=1))
    line("gathers landed med", np.median(landed, axis=1))
    line("gathers landed max", landed.max(axis=1))
    line("slot stored med", np.median(stored, axis=1))
    line("slot stored max", stored.max(axis=1))
    line("finisher entry", a[:, 0, nw] - t0)
    line("finisher has all partials", a[:, 1, nw] - t0)
    line("finisher exit", a[:, 2, nw] - t0)
    line("gathers landed -> slot stored", np.median(stored - landed, axis=1))
    line("finisher holds all -> exit", a[:, 2, nw] - a[:, 1, nw])


if __name__ == "__main__":
    main()
