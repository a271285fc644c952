// kbest_hybrid_sample.hip compiled for the HOST, line for line, as hybrid_dev_host.cpp does for kbest_hybrid.hip: a workgroup is 256
// std::threads, __syncthreads a std::barrier, the wave operations go through per-wave barriers.  Built with
// -fsanitize=address,undefined and run on exact-size heap buffers laid out as kbest_hybrid_frontier_sample_assoc_batch_f64_dev lays
// out its work space, it checks the index arithmetic of the gather, the key kernel and the join before any GPU run: no access
// beyond a buffer, every key, offset and draw where the host loop of kbest_hybrid_frontier_sample_assoc_batch_f64 puts it.  The
// partial kernel's outputs, the clustered sampler's draws and the list sampler's per-cluster outputs come from the Python
// restatement; tests/test_hybrid_sample_dev_cpu.py builds and runs it.
// With a third argument the list sampler is not taken from the restatement: frontier_sample_list_kernel itself
// (kbest_frontier_sample.hip, compiled for the host as in frontier_sample_host.cpp) runs on the gathered list, two workgroups
// striding over it -- the whole device path behind the two clustered kernels, end to end.
// usage: hybrid_sample_dev_host IN OUT [sampler]
//   IN:  int B, maxRawRow, maxCol, condition, maxWidth, nSample; u64 seed; per frame: int nL, nM, info, nOpen; u64 frameKey; the
//        (nL + nM) * nM doubles of its cost block; double logPerm of the partial kernel, of the clustered sampler; int label[nM];
//        the clustered sampler's int assign[nSample][nM] and double logProb[nSample]; per open cluster: int root, m, nL_k, R_k;
//        int rows[nL_k]; int info, width; double logZ; int local[nSample][m]; double term[nSample]; the (nL_k + m) * m doubles of
//        its sub-block.
//   OUT: int count; per cluster of the list: int b, root, m, nL, R, sent; long long subOff, rowKeyOff, asgOff, ltOff; u64 frameKey;
//        its nL + m keys; per frame: int method, nFrontier, nOpen, first; double logPerm; int assign[nSample][nM]; double
//        logProb[nSample].
#include "hip_on_host.h"
#include "kbest_frontier_sample.hip"
#include "kbest_hybrid.hip"
#include "kbest_hybrid_sample.hip"

template <class T> static T get(FILE *f)
{
    T v;
    if (fread(&v, sizeof(T), 1, f) != 1) exit(2);
    return v;
}
template <class T> static void get(FILE *f, T *p, size_t n)
{
    if (n && fread(p, sizeof(T), n, f) != n) exit(2);
}

struct Cluster { int info, width; double logZ; std::vector<int> local; std::vector<double> term, block; };

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    const int B = get<int>(f), maxRawRow = get<int>(f), maxCol = get<int>(f), condition = get<int>(f), maxWidth = get<int>(f),
              nSample = get<int>(f);
    const u64 seed = get<u64>(f);
    std::vector<int> nL(B), nM(B), info(B), nOpen(B), assign;
    std::vector<u64> frameKey(B);
    std::vector<long long> costOff(B), asgOff(B), lpOff(B);
    std::vector<double> cost, logProb, partLp(B), drawLp(B);
    // exact-size heap buffers, strides as the entry's: AddressSanitizer sees any access beyond one
    std::vector<int> label((size_t)B * maxCol, -1), desc((size_t)B * maxCol * 4, -77), rows((size_t)B * maxRawRow, -77);
    std::vector<std::vector<Cluster>> cl(B);
    for (int b = 0; b < B; b++) {
        nL[b] = get<int>(f); nM[b] = get<int>(f); info[b] = get<int>(f); nOpen[b] = get<int>(f); frameKey[b] = get<u64>(f);
        const size_t cn = (size_t)(nL[b] + nM[b]) * nM[b], an = (size_t)nSample * nM[b];
        costOff[b] = (long long)cost.size(); asgOff[b] = (long long)assign.size(); lpOff[b] = (long long)logProb.size();
        cost.resize(cost.size() + cn); assign.resize(assign.size() + an); logProb.resize(logProb.size() + nSample);
        get(f, cost.data() + costOff[b], cn);
        partLp[b] = get<double>(f); drawLp[b] = get<double>(f);
        get(f, label.data() + (size_t)b * maxCol, (size_t)nM[b]);
        get(f, assign.data() + asgOff[b], an);
        get(f, logProb.data() + lpOff[b], (size_t)nSample);
        size_t rowAt = 0;
        for (int j = 0; j < nOpen[b]; j++) {
            int *d = desc.data() + ((size_t)b * maxCol + j) * 4;
            get(f, d, 4);
            get(f, rows.data() + (size_t)b * maxRawRow + rowAt, (size_t)d[2]);
            rowAt += (size_t)d[2];
            Cluster c;
            c.info = get<int>(f); c.width = get<int>(f); c.logZ = get<double>(f);
            c.local.resize((size_t)nSample * d[1]);
            get(f, c.local.data(), c.local.size());
            c.term.resize(nSample);
            get(f, c.term.data(), c.term.size());
            c.block.resize((size_t)(d[2] + d[1]) * d[1]);
            get(f, c.block.data(), c.block.size());
            cl[b].push_back(c);
        }
    }
    fclose(f);
    const long long cap = (long long)B * maxCol, packStride = (long long)maxCol * maxRawRow;
    std::vector<kb::HybridItem> list((size_t)cap);
    std::vector<kb::HybridKeyItem> keys((size_t)cap);
    std::vector<int> first(B, -77), count(1, -77), finfo((size_t)cap, -77), width((size_t)cap, -77);
    std::vector<int> method(B, -77), nFrontier(B, -77), nOpenOut(B, -77), rowKey((size_t)B * maxRawRow, -77);
    std::vector<int> local((size_t)cap * nSample, -77);
    std::vector<double> term((size_t)cap * nSample, -5.0), logZ((size_t)cap, -5.0), logPerm(B, -5.0);
    std::vector<long long> probOff(B, -77);
    memset(list.data(), 0xff, list.size() * sizeof(kb::HybridItem));
    memset(keys.data(), 0xff, keys.size() * sizeof(kb::HybridKeyItem));
    kb::HybridParams hp{};
    hp.nL = nL.data(); hp.nM = nM.data(); hp.costOff = costOff.data(); hp.nOpen = nOpen.data(); hp.openDesc = desc.data();
    hp.list = list.data(); hp.count = count.data(); hp.first = first.data(); hp.packStride = packStride; hp.B = B;
    hp.maxRawRow = maxRawRow; hp.maxCol = maxCol;
    kb::HybridSampleParams p{};
    p.nL = nL.data(); p.nM = nM.data(); p.costOff = costOff.data(); p.asgOff = asgOff.data(); p.lpOff = lpOff.data();
    p.cost = cost.data(); p.frameKey = frameKey.data(); p.assign = assign.data(); p.logProb = logProb.data();
    p.logPerm = logPerm.data(); p.method = method.data(); p.nOpenOut = nOpenOut.data(); p.nFrontier = nFrontier.data();
    p.info = info.data(); p.nOpen = nOpen.data(); p.label = label.data(); p.openDesc = desc.data(); p.openRows = rows.data();
    p.partLogPerm = partLp.data(); p.drawLogPerm = drawLp.data(); p.probOff = probOff.data(); p.list = list.data();
    p.count = count.data(); p.first = first.data(); p.keys = keys.data(); p.rowKey = rowKey.data(); p.local = local.data();
    p.term = term.data(); p.logZ = logZ.data(); p.finfo = finfo.data(); p.width = width.data(); p.packStride = packStride;
    p.B = B; p.maxRawRow = maxRawRow; p.maxCol = maxCol; p.condition = condition; p.maxWidth = maxWidth; p.nSample = nSample;
    kb::launch_hybrid_sample_prepare(p, nullptr);
    for (int b = 0; b < B; b++)
        if (probOff[b] != (long long)b * packStride) return 3;
    kb::launch_hybrid_gather(hp, nullptr);
    kb::launch_hybrid_sample_keys(p, nullptr);
    const bool sampler = argc > 3;
    if (sampler && maxWidth > 0) {  // d_sub as the partial kernel leaves it: shaped like cost, a frame's sub-blocks one after another
        std::vector<double> sub(cost.size(), -7.0);
        for (int b = 0; b < B; b++) {
            size_t at = (size_t)costOff[b];
            for (const Cluster &c : cl[b]) {
                if (at + c.block.size() > sub.size()) return 3;
                memcpy(sub.data() + at, c.block.data(), c.block.size() * 8);
                at += c.block.size();
            }
        }
        const int grid = 2;
        kb::FrontierWork w;
        w.slotDoubles = (4 << 20) / 8; w.planDoubles = (long long)maxRawRow * kb::KB_FRONTIER_STEP_DOUBLES;
        std::vector<double> layers((size_t)w.slotDoubles * grid), plan((size_t)w.planDoubles * grid);
        w.layers = layers.data(); w.plan = plan.data();
        kb::launch_frontier_sample_list(list.data(), keys.data(), count.data(), sub.data(), rowKey.data(), nSample, seed, 0u,
                                        local.data(), term.data(), logZ.data(), finfo.data(), width.data(), w, grid, nullptr);
    }
    // else the sampler's part from the restatement: every sent cluster's outputs where the key items say they go
    for (int b = 0, k = 0; b < B && !sampler; b++)
        for (int j = 0; j < nOpen[b]; j++, k++) {
            if (k >= count[0] || !keys[k].sent) continue;
            const Cluster &c = cl[b][j];
            finfo[k] = c.info; width[k] = c.width; logZ[k] = c.logZ;
            if (keys[k].asgOff < 0 || keys[k].asgOff + (long long)c.local.size() > (long long)local.size() || keys[k].ltOff < 0 ||
                keys[k].ltOff + nSample > (long long)term.size())
                return 3;
            memcpy(local.data() + keys[k].asgOff, c.local.data(), c.local.size() * 4);
            memcpy(term.data() + keys[k].ltOff, c.term.data(), c.term.size() * 8);
        }
    kb::launch_hybrid_sample_join(p, nullptr);
    f = fopen(argv[2], "wb");
    fwrite(count.data(), 4, 1, f);
    for (int k = 0; k < count[0] && k < cap; k++) {
        const kb::HybridItem &it = list[k];
        const kb::HybridKeyItem &ky = keys[k];
        const int six[6] = {it.b, it.root, it.m, it.nL, ky.R, ky.sent};
        const long long four[4] = {it.subOff, ky.rowKeyOff, ky.asgOff, ky.ltOff};
        fwrite(six, 4, 6, f); fwrite(four, 8, 4, f); fwrite(&ky.frameKey, 8, 1, f);
        if (ky.sent) fwrite(rowKey.data() + ky.rowKeyOff, 4, (size_t)(it.nL + it.m), f);
    }
    for (int b = 0; b < B; b++) {
        const int four[4] = {method[b], nFrontier[b], nOpenOut[b], first[b]};
        fwrite(four, 4, 4, f); fwrite(&logPerm[b], 8, 1, f);
        fwrite(assign.data() + asgOff[b], 4, (size_t)nSample * nM[b], f);
        fwrite(logProb.data() + lpOff[b], 8, (size_t)nSample, f);
    }
    fclose(f);
    return 0;
}
