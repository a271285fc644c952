// kbest_factors.hip compiled for the HOST, line for line, as quadric_map_sample_host.cpp does for its kernel: a workgroup is
// block.x std::threads, ballot and mbcnt have the lane semantics of gfx950.  Built with -fsanitize=address,undefined
// -ffp-contract=off and run on exact-size heap buffers -- every list exactly its capacity long, the support exactly nSupport, the
// work space exactly B * maxCol -- it checks the index arithmetic of the count, scan and emit passes before any GPU run: the caller
// hands over every input as it stands before the launch and gets every output back as it stands after it, handed over full of
// sentinels (-77 / -5.0).  tests/test_factors_cpu.py builds and runs it (tests/factors_lib.py writes IN and reads OUT).
// usage: factors_host IN OUT
//   IN:  int B, maxSlot, maxCol, flags (1 rowIdx, 2 landOff, 4 method, 8 support, 16 fMap); long long rowStride, nSupport, maxFactor,
//        maxNew, nProbs; double factorThresh, newThresh, boxSd; long long probOff[B], landOff[B]; int nSlot[B], nM[B], method[B];
//        int rowIdx[B * rowStride] with flag 1; double probs[nProbs].
//   OUT: long long total[2], factorOff[B], newOff[B]; int nFactor[B], nNew[B]; long long fMap[maxFactor] with flag 16; double
//        fProb, fSigma [maxFactor], nProb, nSigma [maxNew]; int fFrame, fMeas, fLand [maxFactor], nFrame, nMeas [maxNew]; int
//        support[nSupport] with flag 8.
#include "hip_on_host.h"
#include "kbest_factors.hip"

template <class T> static T get(FILE *f)
{
    T v;
    if (fread(&v, sizeof(T), 1, f) != 1) exit(2);
    return v;
}
template <class T> static void get(FILE *f, std::vector<T> &v)
{
    if (!v.empty() && fread(v.data(), sizeof(T), v.size(), f) != v.size()) exit(2);
}
template <class T> static void put(FILE *f, const std::vector<T> &v)
{
    if (!v.empty() && fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) exit(2);
}
template <class T> static T *ptr(std::vector<T> &v) { return v.empty() ? nullptr : v.data(); }  // (capacity 0: a counting call)

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    const int B = get<int>(f), maxSlot = get<int>(f), maxCol = get<int>(f), flags = get<int>(f);
    const long long rowStride = get<long long>(f), nSupport = get<long long>(f), maxFactor = get<long long>(f),
                    maxNew = get<long long>(f), nProbs = get<long long>(f);
    const double factorThresh = get<double>(f), newThresh = get<double>(f), boxSd = get<double>(f);
    if (B < 0 || maxSlot < 0 || maxCol < 1 || maxCol > kb::FACTOR_MAX_COLS || rowStride < 0 || nSupport < 0 || maxFactor < 0 ||
        maxNew < 0 || nProbs < 0)
        return 2;
    // exact-size heap buffers: AddressSanitizer sees any access beyond one
    std::vector<long long> probOff(B), landOff(B);
    std::vector<int> nSlot(B), nM(B), method(B), rowIdx((flags & 1) ? (size_t)B * rowStride : 0);
    std::vector<double> probs((size_t)nProbs);
    get(f, probOff);
    get(f, landOff);
    get(f, nSlot);
    get(f, nM);
    get(f, method);
    get(f, rowIdx);
    get(f, probs);
    fclose(f);
    const int IP = -77;
    const double FP = -5.0;
    std::vector<long long> total(2, IP), factorOff(B, IP), newOff(B, IP), fMap((flags & 16) ? (size_t)maxFactor : 0, IP);
    std::vector<int> nFactor(B, IP), nNew(B, IP), fFrame((size_t)maxFactor, IP), fMeas((size_t)maxFactor, IP), fLand((size_t)maxFactor, IP),
        nFrame((size_t)maxNew, IP), nMeas((size_t)maxNew, IP), support((flags & 8) ? (size_t)nSupport : 0, IP),
        rowCnt((size_t)B * maxCol, IP), rowNew((size_t)B * maxCol, IP);
    std::vector<double> fProb((size_t)maxFactor, FP), fSigma((size_t)maxFactor, FP), nProb((size_t)maxNew, FP), nSigma((size_t)maxNew, FP);
    kb::FactorParams p;
    p.probs = ptr(probs); p.probOff = ptr(probOff); p.nSlot = ptr(nSlot); p.nM = ptr(nM);
    p.rowIdx = (flags & 1) ? ptr(rowIdx) : nullptr; p.rowStride = rowStride;
    p.landOff = (flags & 2) ? ptr(landOff) : nullptr; p.method = (flags & 4) ? ptr(method) : nullptr;
    p.factorThresh = factorThresh; p.newThresh = newThresh; p.boxSd = boxSd;
    p.B = B; p.maxSlot = maxSlot; p.maxCol = maxCol; p.maxFactor = maxFactor; p.maxNew = maxNew;
    p.fFrame = ptr(fFrame); p.fMeas = ptr(fMeas); p.fLand = ptr(fLand); p.fMap = ptr(fMap); p.fProb = ptr(fProb); p.fSigma = ptr(fSigma);
    p.nFrame = ptr(nFrame); p.nMeas = ptr(nMeas); p.nProb = ptr(nProb); p.nSigma = ptr(nSigma);
    p.nFactor = ptr(nFactor); p.nNew = ptr(nNew); p.factorOff = ptr(factorOff); p.newOff = ptr(newOff); p.total = ptr(total);
    p.support = (flags & 8) ? ptr(support) : nullptr; p.nSupport = nSupport;
    p.rowCnt = ptr(rowCnt); p.rowNew = ptr(rowNew);
    if (kb::launch_assoc_factors(p, nullptr) != hipSuccess) return 3;
    f = fopen(argv[2], "wb");
    if (!f) return 2;
    put(f, total); put(f, factorOff); put(f, newOff); put(f, nFactor); put(f, nNew); put(f, fMap);
    put(f, fProb); put(f, fSigma); put(f, nProb); put(f, nSigma);
    put(f, fFrame); put(f, fMeas); put(f, fLand); put(f, nFrame); put(f, nMeas); put(f, support);
    fclose(f);
    return 0;
}
