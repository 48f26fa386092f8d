/* C99 caller of gs_trace_contour through include/grayskull.h alone: the struct layout and the reference's own test
 * vector (ref test.c:261-287).  Built -std=c99 -pedantic -Werror by tests/test_contours.py (emulator build) and
 * tests/test_gpu_contours.py (product library). */
#include "grayskull.h"

#include <stddef.h>
#include <stdio.h>
#include <string.h>

#define W 255

int main(void) {
  uint8_t data[5 * 5] = {0, W, W, W, 0, 0, W, W, W, 0, 0, W, 0, W, W, 0, W, W, W, 0, 0, 0, W, 0, W};
  const uint8_t expected[5 * 5] = {0, W, W, W, 0, 0, W, 0, W, 0, 0, W, 0, 0, W, 0, W, 0, W, 0, 0, 0, W, 0, 0};
  uint8_t visited_data[5 * 5] = {0};
  struct gs_image img = {5, 5, NULL}, visited = {5, 5, NULL};
  struct gs_contour c;
  int bad = 0;
  img.data = data, visited.data = visited_data;
  if (sizeof(struct gs_contour) != 28 || offsetof(struct gs_contour, box) != 0 || offsetof(struct gs_contour, start) != 16 ||
      offsetof(struct gs_contour, length) != 24) {
    printf("struct gs_contour: size %u\n", (unsigned)sizeof(struct gs_contour));
    return 1;
  }
  memset(&c, 0xee, sizeof c);
  c.start.x = 1, c.start.y = 0;
  gs_trace_contour(img, visited, &c);
  if (c.length != 10) bad |= 1;
  if (!(c.box.x == 1 && c.box.y == 0 && c.box.w == 4 && c.box.h == 5)) bad |= 2;
  if (!(c.start.x == 1 && c.start.y == 0)) bad |= 4;
  if (memcmp(visited_data, expected, sizeof expected) != 0) bad |= 8;
  if (bad) {
    printf("gs_trace_contour: failed (%d): length %u box %u %u %u %u\n", bad, c.length, c.box.x, c.box.y, c.box.w, c.box.h);
    return 1;
  }
  printf("all passed\n");
  return 0;
}
