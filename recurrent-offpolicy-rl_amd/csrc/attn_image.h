// Address arithmetic of the swizzled row-major LDS images of csrc/attention.hip (struct Img there), as plain constexpr functions so
// that a host program can walk them: tools/attn_image_check.cpp checks that the map is a bijection and prints the bank pattern of a
// wave's row read (ds_read_b128) and transposed read (ds_read_b64_tr_b16) for every head width.
// An image is [rows][hd] bf16; chunk ch (16 bytes) of row `row` lives at chunk position ch ^ swz(hd, row).  The LDS serves 64 banks
// of 4 bytes (256 bytes) per cycle to one lane group: ds_read_b128 in groups of 16 lanes that hold 16 rows of all residues mod 16,
// ds_read_b64_tr_b16 in the two 32-lane halves (4 consecutive rows x 4 consecutive chunks each).
//   hd  32 ( 64-byte rows): 4 rows span the banks; row bits 2..3 move the chunk.
//   hd  64 (128-byte rows): 2 rows span the banks; row bits 1..3 move the chunk.
//   hd 128 (256-byte rows): every row starts at bank 0; a row read needs all four row bits in the chunk position, a transposed read
//                           needs row bits 0..1 in chunk bits 2..3 (its 4 rows take the same 4 chunks): (row & 3) << 2 | (row >> 2) & 3.
#pragma once

namespace resel_attn_image {

constexpr int swz(int hd, int row) {
    return hd == 32 ? ((row >> 2) & 3)
         : hd == 64 ? ((((row >> 1) & 1) << 2) | ((row >> 2) & 3))
                    : (((row & 3) << 2) | ((row >> 2) & 3));
}
constexpr int off(int hd, int row, int ch) { return row * hd * 2 + ((ch ^ swz(hd, row)) << 4); }
// row read of k-step ks: lane (r, hh) takes row r, chunk 2 ks + hh
constexpr int row_off(int hd, int r, int hh, int ks) { return off(hd, r, 2 * ks + hh); }
// transposed read: k-step s2, first / second block of the step (sec), column tile t
constexpr int tr_off(int hd, int lane, int s2, int sec, int t) {
    const int li = lane & 15, dh = (lane >> 4) & 1, hh = lane >> 5;
    const int row = 16 * s2 + 8 * sec + 4 * hh + (li >> 2);
    return off(hd, row, 4 * t + 2 * dh + ((li & 3) >> 1)) + 8 * (li & 1);
}

}  // namespace resel_attn_image
