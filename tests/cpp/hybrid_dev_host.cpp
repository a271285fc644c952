// kbest_hybrid.hip compiled for the HOST, line for line, as frontier_host.cpp does for the sweep: a workgroup is 256 std::threads,
// __syncthreads a std::barrier, the wave minimum goes through a per-wave barrier.  Built with -fsanitize=address,undefined and run
// on exact-size heap buffers laid out as kbest_hybrid_frontier_probs_batch_f64_dev lays out its work space, it checks the index
// arithmetic of the gather and the scatter before any GPU run: no access beyond a buffer, every block where the host loop of
// hybrid_impl puts it.  The partial kernel's outputs and the sweep's per-cluster outputs come from the Python restatement;
// tests/test_hybrid_dev_cpu.py builds and runs it.
// With a third argument the sweep is not taken from the restatement: frontier_list_kernel itself (kbest_frontier.hip, compiled
// for the host as in frontier_host.cpp) runs on the gathered list, two workgroups striding over it -- the whole device path behind
// the partial kernel, end to end.
// usage: hybrid_dev_host IN OUT [sweep]
//   IN:  int B, maxRawRow, maxCol, condition, maxWidth; per frame: int nL, nM, info, nOpen; the (nL + nM) * nM doubles of its cost
//        block; the nM * (nL + 1) doubles the partial kernel left; double logPerm of the partial kernel; int label[nM]; per open
//        cluster: int root, m, nL_k, R_k; int rows[nL_k]; int info, width; double logZ; the m * (nL_k + 1) doubles of its block;
//        the (nL_k + m) * m doubles of its sub-block.
//   OUT: int count; per cluster of the list: int b, root, m, nL, idx, sent; long long subOff, probOff, rowAt; per frame: int method,
//        nFrontier, nOpen, first; double logPerm; its slice.
#include "hip_on_host.h"
#include "kbest_frontier.hip"
#include "kbest_hybrid.hip"

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

struct Cluster { int info, width; double logZ; std::vector<double> probs, block; };

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    const int B = get<int>(f), maxRawRow = get<int>(f), maxCol = get<int>(f), condition = get<int>(f), maxWidth = get<int>(f);
    std::vector<int> nL(B), nM(B), info(B), nOpen(B);
    std::vector<long long> costOff(B), probOff(B);
    std::vector<double> cost, probs, logPerm(B);
    // exact-size heap buffers, strides as the entry's: AddressSanitizer sees any access beyond one
    std::vector<int> label((size_t)B * maxCol, -1), desc((size_t)B * maxCol * 4, -77), rows((size_t)B * maxRawRow, -77);
    std::vector<std::vector<Cluster>> cl(B);
    for (int b = 0; b < B; b++) {
        nL[b] = get<int>(f); nM[b] = get<int>(f); info[b] = get<int>(f); nOpen[b] = get<int>(f);
        const size_t cn = (size_t)(nL[b] + nM[b]) * nM[b], pn = (size_t)nM[b] * (nL[b] + 1);
        costOff[b] = (long long)cost.size(); probOff[b] = (long long)probs.size();
        cost.resize(cost.size() + cn); probs.resize(probs.size() + pn);
        get(f, cost.data() + costOff[b], cn);
        get(f, probs.data() + probOff[b], pn);
        logPerm[b] = get<double>(f);
        get(f, label.data() + (size_t)b * maxCol, (size_t)nM[b]);
        size_t rowAt = 0;
        for (int j = 0; j < nOpen[b]; j++) {
            int *d = desc.data() + ((size_t)b * maxCol + j) * 4;
            get(f, d, 4);
            get(f, rows.data() + (size_t)b * maxRawRow + rowAt, (size_t)d[2]);
            rowAt += (size_t)d[2];
            Cluster c;
            c.info = get<int>(f); c.width = get<int>(f); c.logZ = get<double>(f);
            c.probs.resize((size_t)d[1] * (d[2] + 1));
            get(f, c.probs.data(), c.probs.size());
            c.block.resize((size_t)(d[2] + d[1]) * d[1]);
            get(f, c.block.data(), c.block.size());
            cl[b].push_back(c);
        }
    }
    fclose(f);
    const long long cap = (long long)B * maxCol, packStride = (long long)maxCol * maxRawRow;
    std::vector<kb::HybridItem> list((size_t)cap);
    std::vector<int> first(B, -77), count(1, -77), finfo((size_t)cap, -77), width((size_t)cap, -77);
    std::vector<int> method(B, -77), nFrontier(B, -77), nOpenOut(B, -77);
    std::vector<double> packed((size_t)B * packStride, -5.0), logZ((size_t)cap, -5.0);
    memset(list.data(), 0xff, list.size() * sizeof(kb::HybridItem));
    kb::HybridParams p;
    p.nL = nL.data(); p.nM = nM.data(); p.costOff = costOff.data(); p.probOff = probOff.data(); p.cost = cost.data();
    p.probs = probs.data(); p.logPerm = logPerm.data(); p.method = method.data(); p.nOpenOut = nOpenOut.data();
    p.nFrontier = nFrontier.data(); p.info = info.data(); p.nOpen = nOpen.data(); p.label = label.data(); p.openDesc = desc.data();
    p.openRows = rows.data(); p.list = list.data(); p.count = count.data(); p.first = first.data(); p.packed = packed.data();
    p.logZ = logZ.data(); p.finfo = finfo.data(); p.width = width.data(); p.packStride = packStride; p.B = B;
    p.maxRawRow = maxRawRow; p.maxCol = maxCol; p.condition = condition; p.maxWidth = maxWidth;
    kb::launch_hybrid_gather(p, nullptr);
    const bool sweep = argc > 3;
    if (sweep) {  // d_sub as the partial kernel leaves it: shaped like cost, a frame's sub-blocks one after another from costOff[b]
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
        kb::launch_frontier_list(list.data(), count.data(), sub.data(), packed.data(), logZ.data(), finfo.data(), width.data(), w, grid,
                                 nullptr);
    }
    // else the sweep's part from the restatement: every sent cluster's outputs where the list says they go
    for (int b = 0, k = 0; b < B && !sweep; b++)
        for (int j = 0; j < nOpen[b]; j++, k++) {
            if (k >= count[0] || !list[k].sent) continue;
            finfo[k] = cl[b][j].info; width[k] = cl[b][j].width; logZ[k] = cl[b][j].logZ;
            if (list[k].probOff < 0 || list[k].probOff + (long long)cl[b][j].probs.size() > (long long)packed.size()) return 3;
            memcpy(packed.data() + list[k].probOff, cl[b][j].probs.data(), cl[b][j].probs.size() * 8);
        }
    kb::launch_hybrid_scatter(p, nullptr);
    f = fopen(argv[2], "wb");
    fwrite(count.data(), 4, 1, f);
    for (int k = 0; k < count[0] && k < cap; k++) {
        const kb::HybridItem &it = list[k];
        const int six[6] = {it.b, it.root, it.m, it.nL, it.idx, it.sent};
        const long long three[3] = {it.subOff, it.probOff, it.rowAt};
        fwrite(six, 4, 6, f); fwrite(three, 8, 3, f);
    }
    for (int b = 0; b < B; b++) {
        const int four[4] = {method[b], nFrontier[b], nOpenOut[b], first[b]};
        fwrite(four, 4, 4, f); fwrite(&logPerm[b], 8, 1, f);
        fwrite(probs.data() + probOff[b], 8, (size_t)nM[b] * (nL[b] + 1), f);
    }
    fclose(f);
    return 0;
}
