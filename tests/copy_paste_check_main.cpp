// The host side of mtbt_copy_paste (csrc/copy_paste_check.h: the checks before any launch and the by-value launch table) as a stand-alone
// program, to be built with the address and undefined-behaviour sanitizers and run on the CPU (tests/test_cpu_copy_paste.py does both).  It
// feeds the rejected tables and the degenerate sizes; the device pointers are made-up addresses, which the checks never dereference.
// Prints "copy_paste_check: N cases ok" and returns 0, or names the first case that gave another status and returns 1.
#include <stdio.h>

#include <vector>

#include "copy_paste_check.h"

namespace {

int cases = 0, failures = 0;

struct Call {
  std::vector<int32_t> row_off{0, 2, 3}, paste_off{0, 1, 3};
  std::vector<int32_t> entries{2, 5, -3, 1, 0, 0, 0, 0, /**/ 0, 0, 0, 0, 0, 0, 0, 0, /**/ 1, -64, 64, 1, 0, 0, 0, 0};
  mtbt_copy_paste_args a{};
  Call() {
    auto at = [](uintptr_t v) { return reinterpret_cast<void*>(v); };
    a.images = (const float*)at(0x10000000); a.planes = (const uint8_t*)at(0x20000000); a.rows_in = (const float*)at(0x30000000);
    a.out_images = (float*)at(0x40000000); a.out_planes = (uint8_t*)at(0x50000000); a.out_masks = (float*)at(0x60000000);
    a.rows_out = (float*)at(0x70000000); a.area_before = (uint32_t*)at(0x71000000); a.area = (uint32_t*)at(0x72000000); a.box = (int32_t*)at(0x73000000);
    a.B = 2; a.M = 3; a.P = 3; a.S = 64; a.pitch = 8; a.entry_stride = 8;
  }
  int run() {
    a.row_off = row_off.data(); a.paste_off = paste_off.data(); a.entries = entries.data();
    return copy_paste::check(&a);
  }
};

void expect(const char* what, int got, int want) {
  ++cases;
  if (got != want) {
    ++failures;
    printf("copy_paste_check: %s gave %d, expected %d\n", what, got, want);
  }
}

}  // namespace

int main() {
  { Call c; expect("a valid call", c.run(), MTBT_OK); }
  expect("a NULL struct", copy_paste::check(nullptr), MTBT_EINVAL);
  // the launch table of the valid call: donors found through row_off, an empty canvas in front of the donor included
  {
    Call c;
    c.row_off = {0, 0, 3}; c.paste_off = {0, 1, 3};
    expect("an empty first canvas", c.run(), MTBT_OK);
    copy_paste::Batch b;
    copy_paste::describe(c.a, 0, 2, b);
    expect("describe: entries of canvas 0", b.c[0].n, 1);
    expect("describe: donor canvas of row 2", b.c[0].e[0].src, 1 << 1 | 1);
    expect("describe: entries of canvas 1", b.c[1].n, 2);
    expect("describe: donor canvas of row 0", b.c[1].e[0].src, 1 << 1 | 0);
    expect("describe: rows of canvas 1", b.c[1].row1 - b.c[1].row0, 3);
    expect("describe: an unused slot is zero", b.c[2].n + b.c[7].row1, 0);
  }
  {
    Call c;
    expect("the valid call again", c.run(), MTBT_OK);
    copy_paste::Batch b;
    copy_paste::describe(c.a, 0, 2, b);
    expect("describe: row 2 lies on canvas 1", b.c[0].e[0].src >> 1, 1);
    expect("describe: row 1 lies on canvas 0", b.c[1].e[1].src >> 1, 0);
    expect("describe: dx, dy", b.c[1].e[1].dx * 1000 + b.c[1].e[1].dy, -64 * 1000 + 64);
  }
  // NULL required pointers
  { Call c; c.run(); c.a.row_off = nullptr; expect("NULL row_off", copy_paste::check(&c.a), MTBT_EINVAL); }
  { Call c; c.run(); c.a.paste_off = nullptr; expect("NULL paste_off", copy_paste::check(&c.a), MTBT_EINVAL); }
  { Call c; c.run(); c.a.entries = nullptr; expect("NULL entries", copy_paste::check(&c.a), MTBT_EINVAL); }
  { Call c; c.a.images = nullptr; expect("NULL images", c.run(), MTBT_EINVAL); }
  { Call c; c.a.planes = nullptr; expect("NULL planes", c.run(), MTBT_EINVAL); }
  { Call c; c.a.out_images = nullptr; expect("NULL out_images", c.run(), MTBT_EINVAL); }
  { Call c; c.a.out_planes = nullptr; expect("NULL out_planes", c.run(), MTBT_EINVAL); }
  { Call c; c.a.area_before = nullptr; expect("NULL area_before", c.run(), MTBT_EINVAL); }
  { Call c; c.a.area = nullptr; expect("NULL area", c.run(), MTBT_EINVAL); }
  { Call c; c.a.box = nullptr; expect("NULL box", c.run(), MTBT_EINVAL); }
  { Call c; c.a.rows_in = nullptr; expect("rows_out without rows_in", c.run(), MTBT_EINVAL); }
  { Call c; c.a.rows_in = nullptr; c.a.rows_out = nullptr; expect("no rows at all", c.run(), MTBT_OK); }
  { Call c; c.a.out_masks = nullptr; expect("no mask", c.run(), MTBT_OK); }
  // sizes
  { Call c; c.a.B = -1; expect("B < 0", c.run(), MTBT_EINVAL); }
  { Call c; c.a.M = -1; expect("M < 0", c.run(), MTBT_EINVAL); }
  { Call c; c.a.P = -1; expect("P < 0", c.run(), MTBT_EINVAL); }
  for (int S : {0, -64, 2, 62, 32772, 1 << 20}) { Call c; c.a.S = S; c.a.pitch = 8 * ((S + 63) / 64); expect("S outside the limits", c.run(), MTBT_EINVAL); }
  { Call c; c.a.S = 32768; c.a.pitch = 4096; c.a.images = (const float*)0x100000000000; c.a.planes = (const uint8_t*)0x200000000000; c.a.out_images = (float*)0x8000000000; c.a.out_planes = (uint8_t*)0x9000000000; c.a.out_masks = (float*)0xa000000000;
    expect("the largest canvas", c.run(), MTBT_OK); }
  for (int pitch : {0, 7, 16, -8}) { Call c; c.a.pitch = pitch; expect("a wrong pitch", c.run(), MTBT_EINVAL); }
  { Call c; c.a.S = 96; c.a.pitch = 8; expect("pitch of S = 96", c.run(), MTBT_EINVAL); }
  { Call c; c.a.S = 96; c.a.pitch = 16; expect("S = 96", c.run(), MTBT_OK); }
  for (int stride : {0, 4, 7, 9}) { Call c; c.a.entry_stride = stride; expect("entry_stride != 8", c.run(), MTBT_EINVAL); }
  // offset tables
  { Call c; c.row_off = {1, 2, 3}; expect("row_off starts elsewhere", c.run(), MTBT_EINVAL); }
  { Call c; c.row_off = {0, 3, 2}; expect("row_off decreases and ends elsewhere", c.run(), MTBT_EINVAL); }
  { Call c; c.row_off = {0, 4, 3}; expect("row_off decreases", c.run(), MTBT_EINVAL); }
  { Call c; c.row_off = {0, 2, 2}; expect("row_off ends before M", c.run(), MTBT_EINVAL); }
  { Call c; c.row_off = {0, 2, 4}; expect("row_off ends behind M", c.run(), MTBT_EINVAL); }
  { Call c; c.paste_off = {1, 1, 3}; expect("paste_off starts elsewhere", c.run(), MTBT_EINVAL); }
  { Call c; c.paste_off = {0, 4, 3}; expect("paste_off decreases", c.run(), MTBT_EINVAL); }
  { Call c; c.paste_off = {0, 1, 2}; expect("paste_off ends before P", c.run(), MTBT_EINVAL); }
  { Call c; c.paste_off = {0, -1, 3}; expect("paste_off negative", c.run(), MTBT_EINVAL); }
  {
    Call c;
    c.a.P = 17; c.paste_off = {0, 17, 17}; c.entries.assign(17 * 8, 0);
    expect("17 entries on a canvas", c.run(), MTBT_EINVAL);
    c.a.P = 16; c.paste_off = {0, 16, 16}; c.entries.assign(16 * 8, 0);
    expect("16 entries on a canvas", c.run(), MTBT_OK);
    c.a.P = 32; c.paste_off = {0, 16, 32}; c.entries.assign(32 * 8, 0);
    expect("16 entries on each canvas", c.run(), MTBT_OK);
  }
  // entries: every field, the last entry included (checked in full before any launch)
  for (int e : {0, 2}) {
    { Call c; c.entries[8 * e] = 3; expect("src_row == M", c.run(), MTBT_EINVAL); }
    { Call c; c.entries[8 * e] = -1; expect("src_row < 0", c.run(), MTBT_EINVAL); }
    for (int f : {1, 2})
      for (int v : {65, -65, 1 << 30, -(1 << 30)}) { Call c; c.entries[8 * e + f] = v; expect("an offset outside the limit", c.run(), MTBT_EINVAL); }
    for (int f : {1, 2})
      for (int v : {64, -64}) { Call c; c.entries[8 * e + f] = v; expect("an offset at the limit", c.run(), MTBT_OK); }
    for (int v : {2, -1}) { Call c; c.entries[8 * e + 3] = v; expect("flip outside {0, 1}", c.run(), MTBT_EINVAL); }
    for (int f : {4, 5, 6, 7}) { Call c; c.entries[8 * e + f] = 1; expect("a non-zero reserved field", c.run(), MTBT_EINVAL); }
  }
  // overlap of an output with an input: images 2 * 3 * 64 * 64 * 4 bytes, planes 3 * 64 * 8, rows 3 * 24
  { Call c; c.a.out_images = (float*)((uintptr_t)c.a.images + 98304 - 16); expect("out_images into images", c.run(), MTBT_EINVAL); }
  { Call c; c.a.out_images = (float*)((uintptr_t)c.a.images + 98304); expect("out_images behind images", c.run(), MTBT_OK); }
  { Call c; c.a.out_images = (float*)c.a.images; expect("in place", c.run(), MTBT_EINVAL); }
  { Call c; c.a.out_masks = (float*)((uintptr_t)c.a.images - 16); expect("out_masks into images", c.run(), MTBT_EINVAL); }
  { Call c; c.a.out_planes = (uint8_t*)((uintptr_t)c.a.planes + 1536 - 8); expect("out_planes into planes", c.run(), MTBT_EINVAL); }
  { Call c; c.a.out_planes = (uint8_t*)((uintptr_t)c.a.planes - 3072); expect("out_planes in front of planes", c.run(), MTBT_OK); }
  { Call c; c.a.out_planes = (uint8_t*)((uintptr_t)c.a.planes - 3072 + 8); expect("out_planes reaching planes", c.run(), MTBT_EINVAL); }
  { Call c; c.a.rows_out = (float*)c.a.rows_in; expect("rows_out on rows_in", c.run(), MTBT_EINVAL); }
  { Call c; c.a.box = (int32_t*)((uintptr_t)c.a.rows_in + 68); expect("box into rows_in", c.run(), MTBT_EINVAL); }
  { Call c; c.a.area = (uint32_t*)((uintptr_t)c.a.planes + 4); expect("area into planes", c.run(), MTBT_EINVAL); }
  { Call c; c.a.area_before = (uint32_t*)((uintptr_t)c.a.images + 4); expect("area_before into images", c.run(), MTBT_EINVAL); }
  // alignment comes second
  { Call c; c.a.images = (const float*)((uintptr_t)c.a.images + 8); expect("images not 16-byte aligned", c.run(), MTBT_EALIGN); }
  { Call c; c.a.out_images = (float*)((uintptr_t)c.a.out_images + 4); expect("out_images not 16-byte aligned", c.run(), MTBT_EALIGN); }
  { Call c; c.a.out_masks = (float*)((uintptr_t)c.a.out_masks + 8); expect("out_masks not 16-byte aligned", c.run(), MTBT_EALIGN); }
  { Call c; c.a.planes = (const uint8_t*)((uintptr_t)c.a.planes + 4); expect("planes not 8-byte aligned", c.run(), MTBT_EALIGN); }
  { Call c; c.a.out_planes = (uint8_t*)((uintptr_t)c.a.out_planes + 1); expect("out_planes not 8-byte aligned", c.run(), MTBT_EALIGN); }
  { Call c; c.a.rows_in = (const float*)((uintptr_t)c.a.rows_in + 2); expect("rows_in not 4-byte aligned", c.run(), MTBT_EALIGN); }
  { Call c; c.a.rows_out = (float*)((uintptr_t)c.a.rows_out + 1); expect("rows_out not 4-byte aligned", c.run(), MTBT_EALIGN); }
  { Call c; c.a.area_before = (uint32_t*)((uintptr_t)c.a.area_before + 2); expect("area_before not 4-byte aligned", c.run(), MTBT_EALIGN); }
  { Call c; c.a.area = (uint32_t*)((uintptr_t)c.a.area + 3); expect("area not 4-byte aligned", c.run(), MTBT_EALIGN); }
  { Call c; c.a.box = (int32_t*)((uintptr_t)c.a.box + 2); expect("box not 4-byte aligned", c.run(), MTBT_EALIGN); }
  { Call c; c.a.out_images = (float*)((uintptr_t)c.a.out_images + 4); c.entries[3] = 2; expect("invalid and misaligned", c.run(), MTBT_EINVAL); }
  // degenerate sizes
  {
    Call c;
    c.a.B = 0; c.a.M = 0; c.a.P = 0; c.row_off = {0}; c.paste_off = {0}; c.entries.clear();
    c.a.images = nullptr; c.a.planes = nullptr; c.a.out_images = nullptr; c.a.out_planes = nullptr; c.a.area = nullptr; c.a.area_before = nullptr; c.a.box = nullptr;
    c.a.rows_in = nullptr; c.a.rows_out = nullptr; c.a.out_masks = nullptr;
    expect("B == 0 with nothing else", c.run(), MTBT_OK);
  }
  {
    Call c;
    c.a.M = 0; c.a.P = 0; c.row_off = {0, 0, 0}; c.paste_off = {0, 0, 0}; c.entries.clear();
    c.a.planes = nullptr; c.a.out_planes = nullptr; c.a.area = nullptr; c.a.area_before = nullptr; c.a.box = nullptr; c.a.rows_in = nullptr;
    expect("M == 0 and P == 0: the images alone", c.run(), MTBT_OK);
    copy_paste::Batch b;
    copy_paste::describe(c.a, 0, 2, b);
    expect("describe: nothing on the canvases", b.c[0].n + b.c[1].n + b.c[0].row1 + b.c[1].row1, 0);
    c.a.P = 1; c.paste_off = {0, 1, 1}; c.entries.assign(8, 0);
    c.a.out_planes = (uint8_t*)0x50000000; c.a.area = (uint32_t*)0x72000000; c.a.area_before = (uint32_t*)0x71000000; c.a.box = (int32_t*)0x73000000;
    expect("an entry without a plane to take it from", c.run(), MTBT_EINVAL);
  }
  { Call c; c.a.P = 0; c.paste_off = {0, 0, 0}; c.entries.clear(); expect("P == 0", c.run(), MTBT_OK); }
  {
    Call c;                     // nine canvases: the second launch's table, with its donor in the first
    c.a.B = 9; c.a.M = 1; c.a.P = 1; c.row_off = {0, 1, 1, 1, 1, 1, 1, 1, 1, 1}; c.paste_off = {0, 0, 0, 0, 0, 0, 0, 0, 0, 1}; c.entries.assign(8, 0);
    expect("nine canvases", c.run(), MTBT_OK);
    copy_paste::Batch b;
    copy_paste::describe(c.a, 8, 1, b);
    expect("describe: the ninth canvas pastes from the first", b.c[0].n * 100 + b.c[0].e[0].src, 100);
    expect("describe: the slots behind it are empty", b.c[1].n, 0);
  }
  if (failures) return 1;
  printf("copy_paste_check: %d cases ok\n", cases);
  return 0;
}
