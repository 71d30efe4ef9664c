// Host check of the swizzled LDS images of the cgpt attention kernels (recurrent-offpolicy-rl_amd/csrc/attn_image.h), for every head
// width the kernels are built for.  No GPU: the address functions are constexpr and are walked here exactly as the kernels use them.
//   1. every (row, 16-byte chunk) of a 128-row image maps to a distinct 16-byte slot inside the image (the LDS-DMA staging fills slot
//      by slot and applies the swizzle on the source side: a map that is not a bijection reads or leaves holes, one that leaves the
//      image writes out of bounds);
//   2. every operand read of a wave stays inside its 32-row tile;
//   3. the bank pattern of one wave's row read (ds_read_b128, served in four groups of 16 lanes) and of its transposed read
//      (ds_read_b64_tr_b16, served in the two 32-lane halves) is printed, with the worst number of distinct addresses that meet on
//      one of the 64 four-byte banks within a group.  1 = conflict-free; anything else fails.
// Build and run:  c++ -std=c++17 -O1 -I recurrent-offpolicy-rl_amd/csrc tools/attn_image_check.cpp -o attn_image_check && ./attn_image_check
#include <cstdio>
#include <set>
#include <vector>

#include "attn_image.h"

namespace img = resel_attn_image;

// lane groups that share an LDS cycle
static const std::vector<std::vector<int>>& groups_b128() {
    static const std::vector<std::vector<int>> g = [] {
        std::vector<std::vector<int>> v(4);
        const int lo[2][16] = {{0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27}, {4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31}};
        for (int h = 0; h < 2; ++h)
            for (int k = 0; k < 2; ++k)
                for (int i = 0; i < 16; ++i) v[2 * h + k].push_back(32 * h + lo[k][i]);
        return v;
    }();
    return g;
}
static const std::vector<std::vector<int>>& groups_half() {
    static const std::vector<std::vector<int>> g = [] {
        std::vector<std::vector<int>> v(2);
        for (int l = 0; l < 64; ++l) v[l >> 5].push_back(l);
        return v;
    }();
    return g;
}

// worst number of distinct addresses on one bank within a group; `bytes` per lane from addr[lane]
static int worst_way(const int* addr, int bytes, const std::vector<std::vector<int>>& groups, bool print) {
    int worst = 0;
    for (const auto& g : groups) {
        std::set<int> on_bank[64];
        for (int lane : g)
            for (int b = 0; b < bytes; b += 4) on_bank[((addr[lane] + b) / 4) % 64].insert(addr[lane]);
        if (print) {
            std::printf("      lanes %2d..: slot of lane", g[0]);
            for (int lane : g) std::printf(" %2d", (addr[lane] % 256) / 16);
            std::printf("\n");
        }
        for (const auto& s : on_bank) worst = (int)s.size() > worst ? (int)s.size() : worst;
    }
    return worst;
}

static int check(int hd) {
    const int rows = 128, chunks = hd / 8, rowb = hd * 2, ks_n = hd / 16, nd = hd / 32;
    int bad = 0;
    std::vector<int> seen(rows * chunks, 0);
    for (int r = 0; r < rows; ++r)
        for (int c = 0; c < chunks; ++c) {
            const int o = img::off(hd, r, c);
            if (o < 0 || o % 16 || o / 16 >= rows * chunks) { std::printf("hd %d: (row %d, chunk %d) leaves the image: %d\n", hd, r, c, o); return 1; }
            if (o / rowb != r) { std::printf("hd %d: (row %d, chunk %d) leaves its row\n", hd, r, c); ++bad; }
            ++seen[o / 16];
        }
    for (int s : seen) bad += s != 1;
    std::printf("hd %3d: %d-byte rows, %d slots, %s\n", hd, rowb, rows * chunks, bad ? "NOT a bijection" : "every (row, chunk) has its own slot");

    int addr[64], worst_row = 0, worst_tr = 0;
    std::printf("   row read (ds_read_b128), k-step 0, slot = (byte address mod 256) / 16:\n");
    for (int ks = 0; ks < ks_n; ++ks) {
        for (int l = 0; l < 64; ++l) {
            addr[l] = img::row_off(hd, l & 31, l >> 5, ks);
            bad += addr[l] < 0 || addr[l] + 16 > 32 * rowb;
        }
        const int w = worst_way(addr, 16, groups_b128(), ks == 0);
        worst_row = w > worst_row ? w : worst_row;
    }
    std::printf("   transposed read (ds_read_b64_tr_b16), k-step 0, first block, column tile 0:\n");
    for (int s2 = 0; s2 < 2; ++s2)
        for (int sec = 0; sec < 2; ++sec)
            for (int t = 0; t < nd; ++t) {
                for (int l = 0; l < 64; ++l) {
                    addr[l] = img::tr_off(hd, l, s2, sec, t);
                    bad += addr[l] < 0 || addr[l] % 8 || addr[l] + 8 > 32 * rowb;
                    // the lane's 4 elements are columns 32 t + 16 dh + 4 (li & 3) .. + 3 of row 16 s2 + 8 sec + 4 hh + (li >> 2)
                    const int li = l & 15, row = 16 * s2 + 8 * sec + 4 * (l >> 5) + (li >> 2), col = 32 * t + 16 * ((l >> 4) & 1) + 4 * (li & 3);
                    bad += addr[l] != img::off(hd, row, col / 8) + 2 * (col % 8);
                }
                const int w = worst_way(addr, 8, groups_half(), s2 == 0 && sec == 0 && t == 0);
                worst_tr = w > worst_tr ? w : worst_tr;
            }
    std::printf("   worst over all k-steps / blocks / column tiles: row read %d-way, transposed read %d-way%s\n", worst_row, worst_tr,
                bad ? "  ** address check FAILED **" : "");
    return bad + (worst_row != 1) + (worst_tr != 1);
}

int main() {
    int bad = 0;
    for (int hd : {32, 64, 128}) bad += check(hd);
    std::printf(bad ? "FAILED\n" : "ok\n");
    return bad ? 1 : 0;
}
