"""tests/cpp/engine_host.cpp from python: build (optionally from patched copies of the kernel's text: the mutants), write an input
file, run, read the output.  Used by tests/test_engine_cpu.py.  Nothing is loaded into python."""
import os
import shutil
import struct
import subprocess
import time

import numpy as np

from lane_host_lib import ASAN, CSRC, FILLS, ROOT  # noqa: F401  (the same sanitizer flags and fills as the lane kernel's host build)

# (file, the line as it stands in the product text, the mutant's line): each must be found exactly once
MUTANTS = {
    # a slot-table write: the entry that ends an emission run never gets its state slot into the slot table
    1: ("kbest_engine.hip", "                    slotSid[e] = (unsigned short)(tSplit ? psid : sidFirst);\n", "\n"),
    # LDS re-initialisation: the wave that compacts a node's survivors does not put the node's counter of finished filter parts back
    # to zero, which the next round's "last part compacts" depends on
    2: ("kbest_engine.hip", "            if (lane == 0) ctrl->partsDone[myNode] = 0;\n", "\n"),
    # the state-slot bound: the eager region is handed out up to the last slot of the problem, over the atoms of the a-priori
    # threshold that lie there
    3: ("kbest_engine.hip", "                    slot = sl < maxSid ? sl : -1;\n", "                    slot = sl < nSlots ? sl : -1;\n"),
    # LDS shared by lifetime: the first-step and last-arc minima are not re-armed behind the merge, although they share their LDS with
    # the fresh list's gains and meta words, which the round has just filled.  On random costs NOTHING sees this (it was the first
    # candidate for mutant 2 and survived every case): the minima are only ever lowered (atomicMin), and the bit pattern of a positive
    # gain, or an older minimum, reads as a key BELOW that of any reduced cost -- a child's minimum comes out too small, the child passes
    # the filter where it should have been dropped and its search ends at the bound instead: slower, same answers.  A gain of exactly
    # 0.0 is the exception: its bits are the key that decodes to NaN, "no finite minimum", and the child is dropped.  The case
    # zeros_4x4 (every assignment costs 0) was added for it.
    4: ("kbest_engine.hip",
        "        for (int i = tid; i < spec * 64; i += NT) { lbKey[i] = ~0ull; lbIn[i] = ~0u; }  // the fresh lists are consumed: re-arm the minima\n",
        "\n"),
}


def build(tmp, sanitize=ASAN, mutant=0, opt="-O0"):
    """Compile engine_host.cpp; mutant n: from a copy of the csrc directory's headers and kernel files in which ONE line is replaced."""
    tmp = str(tmp)
    os.makedirs(os.path.join(tmp, "hip"), exist_ok=True)
    open(os.path.join(tmp, "hip", "hip_runtime.h"), "w").close()
    inc = CSRC
    if mutant:
        inc = os.path.join(tmp, "csrc_mutant%d" % mutant)
        os.makedirs(inc, exist_ok=True)
        for name in os.listdir(CSRC):
            if name.endswith(".h") or name in ("kbest_engine.hip", "kbest_merge.hip"):
                shutil.copy(os.path.join(CSRC, name), os.path.join(inc, name))
        name, old, new = MUTANTS[mutant]
        text = open(os.path.join(inc, name)).read()
        assert text.count(old) == 1, (mutant, name)
        open(os.path.join(inc, name), "w").write(text.replace(old, new))
    exe = os.path.join(tmp, "engine_host_m%d" % mutant)
    subprocess.check_call(["g++", "-std=c++20", opt, "-g", *sanitize, "-ffp-contract=off", "-Wno-attributes", "-DENGINE_HOST_MUTANT=%d" % mutant,
                           "-I", tmp, "-I", os.path.join(ROOT, "include"), "-I", inc, "-x", "c++",
                           os.path.join(ROOT, "tests", "cpp", "engine_host.cpp"), "-o", exe, "-lpthread"])
    return exe


def _execute(exe, src, out, env, timeout):
    if os.path.exists(out):
        os.remove(out)
    t0 = time.time()
    try:
        pr = subprocess.run([exe, src, out], stderr=subprocess.PIPE, text=True, env=env, timeout=timeout)
    except subprocess.TimeoutExpired as e:  # (threads that wait for one another for ever: reported, not waited for)
        pr = subprocess.CompletedProcess(e.cmd, -999, None, "no end within %d s" % timeout)
    buf = open(out, "rb").read() if pr.returncode == 0 and os.path.exists(out) else None
    return pr, buf, time.time() - t0


def _header(ints, doubles=()):
    ints = list(ints) + [0] * (32 - len(ints))
    doubles = list(doubles) + [0.0] * (8 - len(doubles))
    return struct.pack("<32i", *ints) + struct.pack("<8d", *doubles)


def run(exe, tmp, costs, maxRow, maxCol, k, *, tie=True, spec=8, waves=8, maximize=False, cutoff=None, flags=0, root=(0, 1), fill=1,
        seed=7, nRow=None, nCol=None, extraStates=8, eager=1024, split=1, relay=None, opt=None, gainCols=0, duals=False, tablesHost=False,
        pushed=False, check=True, env=None, timeout=600):
    """costs: (B, maxRow * maxCol), problem b's nRow x nCol block column-major from the start of its row.  relay = (P, first, step);
    opt = (rho0, rho1, phi, kappa, minPool), None: off (optRho0 = 2).  Returns a dict, or (with check = False) (return code, stderr,
    dict or None)."""
    costs = np.ascontiguousarray(costs, dtype=np.float64)
    B = costs.shape[0]
    assert costs.shape[1] == maxRow * maxCol
    src, out = os.path.join(str(tmp), "engine_in.bin"), os.path.join(str(tmp), "engine_out.bin")
    kk = k + 1 if tie else k
    rho0, rho1, slope, kappa, minPool = 2.0, 0.0, 0.0, 0.0, 0
    if opt is not None:  # (as batch_dev_impl sets them)
        rho0, rho1, phi, kappa, minPool = opt
        slope = float((np.float32(rho1) - np.float32(rho0)) / (np.float32(phi) * np.float32(kk)))
    P, first, step = relay if relay is not None else (1, 0, 0)
    with open(src, "wb") as f:
        f.write(_header([0, B, maxRow, maxCol, int(nRow is not None), k, int(tie), spec, waves, int(maximize), int(cutoff is not None), flags,
                         root[0], root[1], fill, seed, extraStates, eager, split, P, first, step, minPool, gainCols, int(duals),
                         int(tablesHost), int(pushed)],
                        [float(cutoff if cutoff is not None else 0.0), rho0, rho1, slope, kappa]))
        if nRow is not None:
            f.write(np.asarray(nRow, np.int32).tobytes() + np.asarray(nCol, np.int32).tobytes())
        f.write(costs.tobytes())
    pr, buf, secs = _execute(exe, src, out, env, timeout)
    res = None
    if buf is not None:
        head = struct.unpack_from("<8i", buf, 0)
        res = dict(statesPerProblem=head[0], lazyStates=head[1], atomSlots=head[2], maxSid=head[3], lds=head[4], kernelK=head[5],
                   status=head[6], relayImage=head[7], seconds=secs)
        at = 32
        nf = np.zeros(B, np.int32); fl = np.zeros(B, np.int32); tg = np.zeros(B); pu = np.zeros(B, np.int64)
        gain = np.zeros((B, k)); r4c = np.zeros((B, k, maxCol), np.int32); c4r = np.zeros((B, k, maxRow), np.int32)
        for b in range(B):
            nf[b], fl[b] = struct.unpack_from("<2i", buf, at); at += 8
            pu[b] = struct.unpack_from("<q", buf, at)[0]; at += 8
            tg[b] = np.frombuffer(buf, np.float64, 1, at)[0]; at += 8
            gain[b] = np.frombuffer(buf, np.float64, k, at); at += 8 * k
            r4c[b] = np.frombuffer(buf, np.int32, k * maxCol, at).reshape(k, maxCol); at += 4 * k * maxCol
            c4r[b] = np.frombuffer(buf, np.int32, k * maxRow, at).reshape(k, maxRow); at += 4 * k * maxRow
        W = B * max(split, 1)
        wnf = np.zeros(W, np.int32); sid = np.zeros((W, k), np.int32)
        for w in range(W):
            wnf[w] = struct.unpack_from("<i", buf, at)[0]; at += 4
            sid[w] = np.frombuffer(buf, np.int32, k, at); at += 4 * k
        res.update(nf=nf, flags=fl, tieGain=tg, pushed=pu, gain=gain, row4col=r4c, col4row=c4r, wgNf=wnf, slotSid=sid)
        if duals:
            res["dualU"] = np.frombuffer(buf, np.float64, B * maxCol, at).reshape(B, maxCol); at += 8 * B * maxCol
            res["dualV"] = np.frombuffer(buf, np.float64, B * maxRow, at).reshape(B, maxRow); at += 8 * B * maxRow
        if P > 1:
            res["relayWords"] = np.frombuffer(buf, np.uint32, 3 * B, at).reshape(3, B); at += 12 * B
        assert at == len(buf)
    if check:
        assert pr.returncode == 0 and res is not None, (pr.returncode, pr.stderr[-3000:])
        assert res["status"] == 0, res["status"]
        return res
    return pr.returncode, pr.stderr, res


def run_condition(exe, tmp, blocks, maxRow, *, fill=1, seed=7, env=None, timeout=300):
    """blocks: list of (nR, nC) arrays (row, column); packed column-major back to back.  Returns (return code, stderr, dict or None)."""
    B = len(blocks)
    nR = [b.shape[0] for b in blocks]; nC = [b.shape[1] for b in blocks]
    off = np.concatenate([[0], np.cumsum([r * c for r, c in zip(nR, nC)])]).astype(np.int64)
    src, out = os.path.join(str(tmp), "engine_in.bin"), os.path.join(str(tmp), "engine_out.bin")
    with open(src, "wb") as f:
        f.write(_header([1, B, maxRow, fill, seed]))
        f.write(np.asarray(nR, np.int32).tobytes() + np.asarray(nC, np.int32).tobytes() + off[:B].tobytes())
        for b in blocks:
            f.write(np.ascontiguousarray(b.T, dtype=np.float64).tobytes())
    pr, buf, secs = _execute(exe, src, out, env, timeout)
    res = None
    if buf is not None:
        total = int(off[B])
        good = np.frombuffer(buf, np.int32, B, 0); condL = np.frombuffer(buf, np.int32, B, 4 * B)
        ridx = np.frombuffer(buf, np.int32, B * maxRow, 8 * B).reshape(B, maxRow)
        outv = np.frombuffer(buf, np.float64, total, 8 * B + 4 * B * maxRow)
        assert 8 * B + 4 * B * maxRow + 8 * total == len(buf)
        res = dict(goodRows=good, condL=condL, rowIdx=ridx, out=outv, off=off, seconds=secs)
    return pr.returncode, pr.stderr, res


def run_weights(exe, tmp, nL, nM, nf, costs, gain, row4col, *, k, maxCol, maxRow, gate=1, solveRows=0, kUse=0, rowIdx=None, nLout=None,
                fill=1, seed=7, env=None, timeout=300):
    """costs: list of 1-d arrays (the single-column path reads nL + 1 entries of problem b's); gain (B, k); row4col (B, k, maxCol).
    Returns (return code, stderr, dict or None); probs: list of (nM, nLo + 1) arrays."""
    B = len(nL)
    costOff = np.concatenate([[0], np.cumsum([len(c) for c in costs])]).astype(np.int64)
    nLo = [nLout[b] if rowIdx is not None else nL[b] for b in range(B)]
    probOff = np.concatenate([[0], np.cumsum([nM[b] * (nLo[b] + 1) for b in range(B)])]).astype(np.int64)
    src, out = os.path.join(str(tmp), "engine_in.bin"), os.path.join(str(tmp), "engine_out.bin")
    with open(src, "wb") as f:
        f.write(_header([2, B, k, maxCol, maxRow, gate, solveRows, kUse, int(rowIdx is not None), fill, seed, int(costOff[B]), int(probOff[B])]))
        f.write(np.asarray(nL, np.int32).tobytes() + np.asarray(nM, np.int32).tobytes() + np.asarray(nf, np.int32).tobytes())
        f.write(costOff[:B].tobytes() + probOff[:B].tobytes())
        for c in costs:
            f.write(np.ascontiguousarray(c, dtype=np.float64).tobytes())
        f.write(np.ascontiguousarray(gain, dtype=np.float64).tobytes())
        f.write(np.ascontiguousarray(row4col, dtype=np.int32).tobytes())
        if rowIdx is not None:
            f.write(np.ascontiguousarray(rowIdx, dtype=np.int32).tobytes() + np.asarray(nLout, np.int32).tobytes())
    pr, buf, secs = _execute(exe, src, out, env, timeout)
    res = None
    if buf is not None:
        chunk, ldsAcc = struct.unpack_from("<2i", buf, 0)
        nfo = np.frombuffer(buf, np.int32, B, 8)
        pv = np.frombuffer(buf, np.float64, int(probOff[B]), 8 + 4 * B)
        assert 8 + 4 * B + 8 * int(probOff[B]) == len(buf)
        probs = [pv[probOff[b]:probOff[b + 1]].reshape(nM[b], nLo[b] + 1) for b in range(B)]
        res = dict(chunk=chunk, ldsAcc=ldsAcc, nf=nfo, probs=probs, seconds=secs)
    return pr.returncode, pr.stderr, res
