// aa_index_host_check.cpp -- the words pass of the amino-acid index builder (blkidx_tile_last_a / blkidx_words_a,
// spaln_amd/csrc/spdp_blk_build.hip) emulated on the CPU: the same tiles of 4096 residues with a halo of 32 classes, the same 256
// threads of 16 residues, the same prefix maximum of "last ambiguous residue" (a thread's own, the shuffle scan of its wave, the
// waves before it, the tile carry of the host loop), the same walk along the sequence offsets -- and the product's per-residue rule
// itself, spdp_blk_build_a.h, compiled for the host.  A program with its own main, built with -fsanitize=address,undefined by
// tests/test_aa_index_host.py: every buffer a thread indexes is a heap block of the kernel's size, so a read the kernel would make
// outside its LDS arrays is reported here.
//
// in : R nalpha weight width spaced nshift exam[weight] / T cls[32] / S n_seq off[n_seq + 1] / C G codes[G]   (one case per file;
//      the codes are what the device sees: residues the scan skips are gone)
// out: "T word count" for every counted word, "K word block" for every (word, block) key, sorted and unique
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>
#include "../spaln_amd/csrc/spdp_blk_build_a.h"

namespace {
constexpr int TILE = 4096, TPB = 256, PER = TILE / TPB, HALO = 32, WAVE = 64;

long long next_int(FILE* f)
{
    long long v = 0;
    if (fscanf(f, "%lld", &v) != 1) { fprintf(stderr, "short input\n"); exit(2); }
    return v;
}
void expect(FILE* f, char tag)
{
    char c = 0;
    if (fscanf(f, " %c", &c) != 1 || c != tag) { fprintf(stderr, "expected %c\n", tag); exit(2); }
}
}   // namespace

int main(int argc, char** argv)
{
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "r");
    if (!f) return 2;
    BlkRuleA R{};
    expect(f, 'R');
    R.nalpha = (int) next_int(f); R.weight = (int) next_int(f); R.width = (int) next_int(f); R.spaced = (int) next_int(f); R.nshift = (int) next_int(f);
    if (R.weight < 1 || R.weight > BLKA_MAX_K || R.width < R.weight || R.width > HALO || R.nshift < 1 || R.nalpha < 2 || R.nalpha > 20) return 2;
    for (int e = 0; e < R.weight; ++e) R.exam[e] = (int) next_int(f);
    expect(f, 'T');
    for (int c = 0; c < 32; ++c) R.cls[c] = (uint8_t) next_int(f);
    expect(f, 'S');
    const int n_seq = (int) next_int(f);
    std::vector<int64_t> seq_off((size_t) n_seq + 1);
    for (auto& x : seq_off) x = next_int(f);
    expect(f, 'C');
    const int64_t G = next_int(f);
    std::vector<uint8_t> codes((size_t) G);
    for (auto& x : codes) x = (uint8_t) next_int(f);
    fclose(f);
    if (n_seq < 1 || seq_off[0] != 0 || seq_off[n_seq] != G) return 2;
    uint64_t tabsize = 1;
    for (int e = 0; e < R.weight; ++e) tabsize *= (uint64_t) R.nalpha;

    const int64_t n_tiles = (G + TILE - 1) / TILE;
    // ---- blkidx_tile_last_a + the host's carry
    std::vector<int64_t> carry((size_t) n_tiles);
    {
        int64_t run = -1;
        for (int64_t t = 0; t < n_tiles; ++t) {
            int64_t last = -1;
            for (int tid = 0; tid < TPB; ++tid)
                for (int i = tid; i < TILE; i += TPB) {
                    const int64_t g = t * TILE + i;
                    if (g < G && blka_class(R.cls, R.nalpha, codes[(size_t) g]) == R.nalpha && g > last) last = g;
                }
            carry[(size_t) t] = run;
            if (last > run) run = last;
        }
    }
    // ---- blkidx_words_a
    std::vector<uint32_t> tcount((size_t) tabsize, 0);
    std::vector<uint64_t> keys;
    for (int64_t t = 0; t < n_tiles; ++t) {
        const int64_t t0 = t * TILE;
        std::unique_ptr<uint8_t[]> s_x(new uint8_t[HALO + TILE]);                 // (exactly the kernel's LDS array)
        for (int i = 0; i < HALO + TILE; ++i) {
            const int64_t g = t0 - HALO + i;
            s_x[i] = (g >= 0 && g < G) ? (uint8_t) blka_class(R.cls, R.nalpha, codes[(size_t) g]) : (uint8_t) R.nalpha;
        }
        int64_t incl[TPB], s_wave[TPB / WAVE];
        for (int tid = 0; tid < TPB; ++tid) {
            const int64_t p0 = t0 + (int64_t) tid * PER;
            int64_t mine = -1;
            for (int i = 0; i < PER; ++i) if (s_x[HALO + tid * PER + i] == R.nalpha && p0 + i < G) mine = p0 + i;
            incl[tid] = mine;
        }
        for (int w = 0; w < TPB / WAVE; ++w) {                                      // the shuffle scan, step by step
            for (int o = 1; o < WAVE; o <<= 1) {
                int64_t before[WAVE];
                for (int l = 0; l < WAVE; ++l) before[l] = incl[w * WAVE + l];
                for (int l = o; l < WAVE; ++l) if (before[l - o] > incl[w * WAVE + l]) incl[w * WAVE + l] = before[l - o];
            }
            s_wave[w] = incl[w * WAVE + WAVE - 1];
        }
        for (int tid = 0; tid < TPB; ++tid) {
            const int lane = tid & (WAVE - 1), wave = tid / WAVE;
            const int64_t p0 = t0 + (int64_t) tid * PER;
            int64_t last = carry[(size_t) t];
            for (int w = 0; w < wave; ++w) last = s_wave[w] > last ? s_wave[w] : last;
            if (lane > 0 && incl[tid - 1] > last) last = incl[tid - 1];
            int c = 0;
            {
                int lo = 0, hi = n_seq;
                while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (seq_off[(size_t) mid] <= p0) lo = mid; else hi = mid; }
                c = lo;
            }
            int64_t c_lo = seq_off[(size_t) c], c_hi = seq_off[(size_t) c + 1];
            for (int i = 0; i < PER; ++i) {
                const int64_t g = p0 + i;
                const bool in = g < G;
                if (in) while (g >= c_hi && c + 1 < n_seq) { ++c; c_lo = c_hi; c_hi = seq_off[(size_t) c + 1]; }
                const int xi = HALO + tid * PER + i;
                if (in && s_x[xi] == R.nalpha) last = g;
                const BlkWordA o = blka_word(R, s_x.get() + xi, g, c_lo, last);
                if (in && o.flawless) {
                    if (o.word >= tabsize) { fprintf(stderr, "word %u beyond the table\n", o.word); return 1; }
                    ++tcount[o.word];
                }
                if (in && o.emit) keys.push_back(((uint64_t) o.word << 32) | (uint32_t) (c + 1));
            }
        }
    }
    std::sort(keys.begin(), keys.end());
    keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
    for (uint64_t w = 0; w < tabsize; ++w) if (tcount[(size_t) w]) printf("T %llu %u\n", (unsigned long long) w, tcount[(size_t) w]);
    for (uint64_t k : keys) printf("K %u %u\n", (uint32_t) (k >> 32), (uint32_t) k);
    return 0;
}
