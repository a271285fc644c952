// kbest_quadric_map_sample.hip compiled for the HOST, line for line, as quadric_map_host.cpp does for the passes over the map: a
// workgroup is 256 std::threads.  Built with -fsanitize=address,undefined -ffp-contract=off and run on exact-size heap buffers, it
// checks the index arithmetic of the kernel that maps compact rows to raw rows before any GPU run: the caller hands over every
// buffer as it stands before the launch and gets assign and logProb back as they stand after it.  It also holds the kernel's frame
// predicate against qmap_frame of kbest_quadric_map.hip on every frame.  tests/test_quadric_map_sample_cpu.py builds and runs it.
// usage: quadric_map_sample_host IN OUT
//   IN:  int B, maxMap, maxKeep, maxCol, nSample, nTiles; long long nAsg, nLp; per frame: long long landOff, measOff, asgOff,
//        lpOff; int nL, nM, nKeep, 0; then int rowIdx[B * maxKeep], int assign[nAsg], double logProb[nLp].
//   OUT: int assign[nAsg]; double logProb[nLp].
#include "hip_on_host.h"
#include "kbest_quadric_map.hip"
#include "kbest_quadric_map_sample.hip"

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
    const int B = get<int>(f), maxMap = get<int>(f), maxKeep = get<int>(f), maxCol = get<int>(f), nSample = get<int>(f),
              nTiles = get<int>(f);
    const long long nAsg = get<long long>(f), nLp = get<long long>(f);
    if (B < 1 || maxMap < 1 || maxKeep < 1 || maxCol < 1 || nSample < 1 || nTiles < 1 || nAsg < 0 || nLp < 0) return 2;
    // exact-size heap buffers: AddressSanitizer sees any access beyond one
    std::vector<long long> landOff(B), measOff(B), asgOff(B), lpOff(B);
    std::vector<int> nL(B), nM(B), nKeep(B), rowIdx((size_t)B * maxKeep), assign((size_t)nAsg);
    std::vector<double> logProb((size_t)nLp);
    for (int b = 0; b < B; b++) {
        landOff[b] = get<long long>(f);
        measOff[b] = get<long long>(f);
        asgOff[b] = get<long long>(f);
        lpOff[b] = get<long long>(f);
        nL[b] = get<int>(f);
        nM[b] = get<int>(f);
        nKeep[b] = get<int>(f);
        (void)get<int>(f);
    }
    get(f, rowIdx.data(), rowIdx.size());
    get(f, assign.data(), assign.size());
    get(f, logProb.data(), logProb.size());
    fclose(f);
    kb::QuadricMapSampleParams p;
    p.landOff = landOff.data(); p.measOff = measOff.data(); p.nL = nL.data(); p.nM = nM.data();
    p.B = B; p.maxMap = maxMap; p.maxKeep = maxKeep; p.maxCol = maxCol; p.nTiles = nTiles; p.nSample = nSample;
    p.nKeep = nKeep.data(); p.rowIdx = rowIdx.data(); p.assign = assign.data(); p.asgOff = asgOff.data();
    p.logProb = logProb.data(); p.lpOff = lpOff.data();
    // one predicate in two files: the same answer on every frame whose draws have a place
    kb::QuadricMapParams g{};
    g.landOff = landOff.data(); g.measOff = measOff.data(); g.nL = nL.data(); g.nM = nM.data();
    g.maxMap = maxMap; g.maxCol = maxCol;
    for (int b = 0; b < B; b++) {
        int l0, m0, l1, m1;
        const bool gate = kb::qmap_frame(g, b, l0, m0), mine = kb::qmap_sample_frame(p, b, l1, m1);
        if (asgOff[b] >= 0 && lpOff[b] >= 0 && (gate != mine || l0 != l1 || m0 != m1)) return 3;
    }
    kb::launch_quadric_map_sample_rows(p, nullptr);
    f = fopen(argv[2], "wb");
    if (!f) return 2;
    fwrite(assign.data(), 4, assign.size(), f);
    fwrite(logProb.data(), 8, logProb.size(), f);
    fclose(f);
    return 0;
}
