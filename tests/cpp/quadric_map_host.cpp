// kbest_quadric_map.hip compiled for the HOST, line for line, as hybrid_dev_host.cpp does for the gather and the scatter: a workgroup
// is 256 std::threads, __syncthreads a std::barrier, the ballot and the wave minimum go through per-wave barriers.  Built with
// -fsanitize=address,undefined -ffp-contract=off and run on exact-size heap buffers laid out as
// kbest_quadric_map_probs_batch_f64_dev lays out its work space, it checks the index arithmetic of the passes before any GPU run and
// the bits of what they compute: nKeep, rowIdx and the compact block against the numpy restatement (tests/quadric_map_lib.py), and
// the expansion on compact probabilities that are their own index.  tests/test_quadric_map_cpu.py builds and runs it.
// usage: quadric_map_host IN OUT
//   IN:  int B, maxMap, maxKeep, maxCol, nMap; double gate; nMap * 3 means; nMap * 9 covariances; per frame: long long landOff;
//        int nL, nM; nM * 3 means; nM * 9 covariances.
//   OUT: per frame: int nKeep, nLh; long long costOff, cprobOff; int rowIdx[maxKeep]; its (maxKeep + maxCol) * maxCol doubles of the
//        compact blocks' buffer (-7.0 where nothing was written); then the whole dense buffer: per frame a pad of 8 doubles and the
//        [nM][nL + 1] slice (-5.0 where nothing was written), and a last pad.
#include "hip_on_host.h"
#include "kbest_quadric_map.hip"

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

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    const int B = get<int>(f), maxMap = get<int>(f), maxKeep = get<int>(f), maxCol = get<int>(f), nMap = get<int>(f);
    const double gate = get<double>(f);
    if (B < 1 || maxMap < 1 || maxKeep < 1 || maxCol < 1 || maxCol > kb::QMAP_MAX_COLS || nMap < 0) return 2;
    // exact-size heap buffers, strides as the entry's: AddressSanitizer sees any access beyond one
    std::vector<double> mapMean((size_t)nMap * 3), mapCov((size_t)nMap * 9), measMean, measCov;
    get(f, mapMean.data(), mapMean.size());
    get(f, mapCov.data(), mapCov.size());
    std::vector<long long> landOff(B), measOff(B), probOff(B);
    std::vector<int> nL(B), nM(B);
    const size_t PAD = 8;
    size_t probN = 0;
    for (int b = 0; b < B; b++) {
        landOff[b] = get<long long>(f);
        nL[b] = get<int>(f);
        nM[b] = get<int>(f);
        const size_t m = nM[b] > 0 ? (size_t)nM[b] : 0;
        measOff[b] = (long long)(measMean.size() / 3);
        measMean.resize(measMean.size() + m * 3);
        measCov.resize(measCov.size() + m * 9);
        get(f, measMean.data() + (size_t)measOff[b] * 3, m * 3);
        get(f, measCov.data() + (size_t)measOff[b] * 9, m * 9);
        probOff[b] = (long long)(probN + PAD);
        probN += PAD + (nL[b] >= 0 ? m * ((size_t)nL[b] + 1) : 0);
    }
    probN += PAD;
    fclose(f);
    kb::QuadricMapParams p;
    const int nTiles = (maxMap + kb::QMAP_TILE - 1) / kb::QMAP_TILE, nKeepTiles = (maxKeep + kb::QMAP_TILE - 1) / kb::QMAP_TILE;
    const size_t costStride = (size_t)(maxKeep + maxCol) * maxCol, cprobStride = (size_t)maxCol * (maxKeep + 1);
    std::vector<double> tileMin((size_t)B * nTiles * maxCol, -7.0), colMin((size_t)B * maxCol, -7.0), ccost((size_t)B * costStride, -7.0);
    std::vector<double> cprobs((size_t)B * cprobStride), probs(probN, -5.0);
    std::vector<u64> keep((size_t)B * nTiles * (kb::QMAP_TILE / 64), ~0ull);
    std::vector<int> tileCnt((size_t)B * nTiles, -77), tileOff((size_t)B * nTiles, -77), nKeep(B, -77), nLh(B, -77), rowIdx((size_t)B * maxKeep, -77);
    std::vector<long long> costOff(B, -77), cprobOff(B, -77);
    for (size_t i = 0; i < cprobs.size(); i++) cprobs[i] = (double)(i + 1);
    p.mapMean = mapMean.data(); p.mapCov = mapCov.data(); p.measMean = measMean.data(); p.measCov = measCov.data();
    p.landOff = landOff.data(); p.measOff = measOff.data(); p.nL = nL.data(); p.nM = nM.data(); p.gate = gate;
    p.B = B; p.maxMap = maxMap; p.maxKeep = maxKeep; p.maxCol = maxCol; p.nTiles = nTiles; p.nKeepTiles = nKeepTiles; p.nExpandTiles = 3;
    p.tileMin = tileMin.data(); p.colMin = colMin.data(); p.keep = keep.data(); p.tileCnt = tileCnt.data(); p.tileOff = tileOff.data();
    p.nKeep = nKeep.data(); p.nLh = nLh.data(); p.costOff = costOff.data(); p.cprobOff = cprobOff.data(); p.rowIdx = rowIdx.data();
    p.ccost = ccost.data(); p.cprobs = cprobs.data(); p.probs = probs.data(); p.probOff = probOff.data();
    kb::launch_quadric_map_gate(p, nullptr);
    kb::launch_quadric_map_fill(p, nullptr);
    kb::launch_quadric_map_expand(p, nullptr);
    f = fopen(argv[2], "wb");
    if (!f) return 2;
    for (int b = 0; b < B; b++) {
        const int two[2] = {nKeep[b], nLh[b]};
        const long long off[2] = {costOff[b], cprobOff[b]};
        fwrite(two, 4, 2, f);
        fwrite(off, 8, 2, f);
        fwrite(rowIdx.data() + (size_t)b * maxKeep, 4, (size_t)maxKeep, f);
        fwrite(ccost.data() + (size_t)b * costStride, 8, costStride, f);
    }
    fwrite(probs.data(), 8, probs.size(), f);
    fclose(f);
    return 0;
}
