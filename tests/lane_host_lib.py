"""tests/cpp/lane_host.cpp from python: build (optionally from patched copies of the kernel's text: the mutants), write an input file,
run, read the output.  Used by tests/test_lane_cpu.py; TSAN is the build of the one-off runs of NOTES section 35."""
import os
import shutil
import struct
import subprocess
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "probabilisticsemslam_amd", "csrc")
ASAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
TSAN = ["-fsanitize=thread"]
FILLS = (1, 2, 3)  # 0x00, 0xFF, seeded bytes

# (file, the line as it stands in the product text, the mutant's line): each must be found exactly once
MUTANTS = {
    # the entry that ends an emission run never gets its state slot into the slot table
    1: ("kbest_lane.hip", "                    slotSid[e] = (unsigned short)(tSplit ? psid : sid0);\n", "\n"),
    # a lane group that draws a new child keeps the shortestPathCost of the child before
    2: ("kbest_lane.hip", "                        for (int r = 0; r < RL; r++) spc[r] = got ? INF : spc[r];\n",
        "                        for (int r = 0; r < RL; r++) spc[r] = spc[r];\n"),
    # the stack of free state slots is sized without the children of a round (k + 2 entries): its upper entries lie in the scratch
    # of the finishing pass behind it.  (ONE entry short cannot be caught by anything: the stack has lane_states_per_problem entries,
    # phase 0 puts one fewer on it -- the root keeps its slot -- and the top one is taken before the scratch is first written.)
    3: ("kbest_engine.h", "    L.offFree = o;     o += lane_states_per_problem(k, spec, maxCol) * 2;  // stack of free state slots\n",
        "    L.offFree = o;     o += lane_states_per_problem(k, 0, maxCol) * 2;\n"),
}


def build(tmp, sanitize=ASAN, mutant=0, opt="-O1"):
    """Compile lane_host.cpp; mutant n: from a copy of the csrc directory's headers and kernel files in which ONE line is replaced."""
    tmp = str(tmp)
    os.makedirs(os.path.join(tmp, "hip"), exist_ok=True)
    open(os.path.join(tmp, "hip", "hip_runtime.h"), "w").close()
    inc = CSRC
    if mutant:
        inc = os.path.join(tmp, "csrc_mutant%d" % mutant)
        os.makedirs(inc, exist_ok=True)
        for name in os.listdir(CSRC):
            if name.endswith(".h") or name in ("kbest_lane.hip", "kbest_merge.hip"):
                shutil.copy(os.path.join(CSRC, name), os.path.join(inc, name))
        name, old, new = MUTANTS[mutant]
        text = open(os.path.join(inc, name)).read()
        assert text.count(old) == 1, (mutant, name)
        open(os.path.join(inc, name), "w").write(text.replace(old, new))
    exe = os.path.join(tmp, "lane_host_m%d" % mutant)
    subprocess.check_call(["g++", "-std=c++20", opt, "-g", *sanitize, "-ffp-contract=off", "-Wno-attributes", "-DLANE_HOST_MUTANT=%d" % mutant,
                           "-I", tmp, "-I", os.path.join(ROOT, "include"), "-I", inc, "-x", "c++",
                           os.path.join(ROOT, "tests", "cpp", "lane_host.cpp"), "-o", exe, "-lpthread"])
    return exe


def run(exe, tmp, costs, maxRow, maxCol, k, *, tie=True, spec=12, waves=4, maximize=False, cutoff=None, flags=0, root=(0, 1), fill=1,
        seed=7, nRow=None, nCol=None, check=True, env=None, timeout=300):
    """costs: (B, maxRow * maxCol), problem b's nRow x nCol block column-major from the start of its row.  Returns a dict, or (with
    check = False) (return code, stderr, dict or None)."""
    costs = np.ascontiguousarray(costs, dtype=np.float64)
    B = costs.shape[0]
    assert costs.shape[1] == maxRow * maxCol
    src, out = os.path.join(str(tmp), "lane_in.bin"), os.path.join(str(tmp), "lane_out.bin")
    with open(src, "wb") as f:
        f.write(struct.pack("<16i", B, maxRow, maxCol, int(nRow is not None), k, int(tie), spec, waves, int(maximize), int(cutoff is not None),
                            flags, root[0], root[1], fill, seed, 0))
        f.write(struct.pack("<d", float(cutoff if cutoff is not None else 0.0)))
        if nRow is not None:
            f.write(np.asarray(nRow, np.int32).tobytes() + np.asarray(nCol, np.int32).tobytes())
        f.write(costs.tobytes())
    if os.path.exists(out):
        os.remove(out)
    t0 = time.time()
    try:
        pr = subprocess.run([exe, src, out], stderr=subprocess.PIPE, text=True, env=env, timeout=timeout)
    except subprocess.TimeoutExpired as e:  # (threads that wait for one another for ever: reported, not waited for)
        pr = subprocess.CompletedProcess(e.cmd, -999, None, "no end within %d s" % timeout)
    res = None
    if pr.returncode == 0 and os.path.exists(out):
        buf = open(out, "rb").read()
        head = struct.unpack_from("<6i", buf, 0)
        res = dict(statesPerProblem=head[0], offFreshG=head[1], offFree=head[2], lds=head[3], kernelK=head[4], status=head[5],
                   seconds=time.time() - t0)
        at = 24
        nf = np.zeros(B, np.int32); fl = np.zeros(B, np.int32); tg = np.zeros(B)
        gain = np.zeros((B, k)); r4c = np.zeros((B, k, maxCol), np.int32); c4r = np.zeros((B, k, maxRow), np.int32)
        sid = np.zeros((B, k), np.int32)
        for b in range(B):
            nf[b], fl[b] = struct.unpack_from("<2i", buf, at); at += 8
            tg[b] = np.frombuffer(buf, np.float64, 1, at)[0]; at += 8
            gain[b] = np.frombuffer(buf, np.float64, k, at); at += 8 * k
            r4c[b] = np.frombuffer(buf, np.int32, k * maxCol, at).reshape(k, maxCol); at += 4 * k * maxCol
            c4r[b] = np.frombuffer(buf, np.int32, k * maxRow, at).reshape(k, maxRow); at += 4 * k * maxRow
            sid[b] = np.frombuffer(buf, np.int32, k, at); at += 4 * k
        assert at == len(buf)
        res.update(nf=nf, flags=fl, tieGain=tg, gain=gain, row4col=r4c, col4row=c4r, slotSid=sid)
    if check:
        assert pr.returncode == 0 and res is not None, (pr.returncode, pr.stderr[-3000:])
        assert res["status"] == 0, res["status"]
        return res
    return pr.returncode, pr.stderr, res
