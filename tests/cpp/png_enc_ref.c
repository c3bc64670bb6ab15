/* png_enc_ref.c -- TEST INFRASTRUCTURE: the write side of the system's libpng (libpng16.so.16, bound by hand like png_ref.c: the
 * image has the library but not its headers), driven the way cv::imencode(".png", img) of OpenCV 3.2 drives it without parameters
 * (modules/imgcodecs/src/grfmt_png.cpp, PngEncoder::write): png_create_write_struct, a memory write function,
 * png_set_filter(PNG_FILTER_TYPE_BASE, PNG_FILTER_SUB), png_set_compression_level(Z_BEST_SPEED),
 * png_set_compression_strategy(Z_RLE), png_set_IHDR (8 bits, gray or RGB, no interlace), png_write_info, png_set_bgr,
 * png_write_image, png_write_end.  The GPU PNG encoder must write the same FILES.
 *     gcc -O2 -shared -fPIC tests/cpp/png_enc_ref.c -o <out>.so -l:libpng16.so.16 */
#include <setjmp.h>
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

typedef void* png_structp;
typedef void* png_infop;
extern png_structp png_create_write_struct(const char* ver, void* error_ptr, void (*error_fn)(png_structp, const char*),
                                           void (*warn_fn)(png_structp, const char*));
extern png_infop png_create_info_struct(png_structp);
extern void png_destroy_write_struct(png_structp*, png_infop*);
extern jmp_buf* png_set_longjmp_fn(png_structp, void (*)(jmp_buf, int), size_t);
extern void png_set_write_fn(png_structp, void* io_ptr, void (*write_fn)(png_structp, unsigned char*, size_t),
                             void (*flush_fn)(png_structp));
extern void* png_get_io_ptr(png_structp);
extern void png_set_filter(png_structp, int method, int filters);
extern void png_set_compression_level(png_structp, int level);
extern void png_set_compression_strategy(png_structp, int strategy);
extern void png_set_IHDR(png_structp, png_infop, uint32_t w, uint32_t h, int depth, int color, int interlace, int comp, int filter);
extern void png_write_info(png_structp, png_infop);
extern void png_set_bgr(png_structp);
extern void png_write_image(png_structp, unsigned char** rows);
extern void png_write_end(png_structp, png_infop);
extern void png_longjmp(png_structp, int);
extern const char* png_get_libpng_ver(png_structp);

typedef struct {
  unsigned char* data;
  size_t size, cap;
  int failed;
} Sink;

static void write_to_buffer(png_structp png, unsigned char* src, size_t n) {
  Sink* s = (Sink*)png_get_io_ptr(png);
  if (s->size + n > s->cap) {
    size_t cap = s->cap ? s->cap : 4096;
    while (cap < s->size + n) cap *= 2;
    unsigned char* p = (unsigned char*)realloc(s->data, cap);
    if (!p) {
      s->failed = 1;
      return;
    }
    s->data = p;
    s->cap = cap;
  }
  memcpy(s->data + s->size, src, n);
  s->size += n;
}
static void flush_nothing(png_structp png) { (void)png; }
static void quiet(png_structp png, const char* msg) {
  (void)png;
  (void)msg;
}
static void failed(png_structp png, const char* msg) {
  (void)msg;
  png_longjmp(png, 1);
}

const char* png_enc_ref_version(void) { return png_get_libpng_ver(NULL); }

/* -> the file's size (its bytes in out[0 .. size), when size <= cap), 0: libpng refused, -1: bad arguments.  src: rows of `pitch`
 * bytes, `channels` (1: gray, 3: B G R) bytes per pixel. */
long png_enc_ref(const unsigned char* src, int width, int height, int channels, size_t pitch, unsigned char* out, size_t cap) {
  if (!src || width < 1 || height < 1 || (channels != 1 && channels != 3) || pitch < (size_t)width * channels) return -1;
  Sink sink = {NULL, 0, 0, 0};
  png_structp png = png_create_write_struct(png_get_libpng_ver(NULL), NULL, failed, quiet);
  png_infop info = png ? png_create_info_struct(png) : NULL;
  unsigned char** volatile rows = (unsigned char**)malloc(sizeof(unsigned char*) * (size_t)height);
  if (!png || !info || !rows) {
    free(rows);
    return 0;
  }
  if (setjmp(*png_set_longjmp_fn(png, longjmp, sizeof(jmp_buf)))) {
    png_destroy_write_struct(&png, &info);
    free(rows);
    free(sink.data);
    return 0;
  }
  png_set_write_fn(png, &sink, write_to_buffer, flush_nothing);
  png_set_filter(png, 0 /* PNG_FILTER_TYPE_BASE */, 0x10 /* PNG_FILTER_SUB */);
  png_set_compression_level(png, 1 /* Z_BEST_SPEED */);
  png_set_compression_strategy(png, 3 /* Z_RLE */);
  png_set_IHDR(png, info, (uint32_t)width, (uint32_t)height, 8, channels == 1 ? 0 /* GRAY */ : 2 /* RGB */, 0, 0, 0);
  png_write_info(png, info);
  png_set_bgr(png);
  for (int y = 0; y < height; y++) rows[y] = (unsigned char*)src + (size_t)y * pitch;
  png_write_image(png, rows);
  png_write_end(png, info);
  png_destroy_write_struct(&png, &info);
  free(rows);
  const long size = sink.failed ? 0 : (long)sink.size;
  if (out && size > 0 && sink.size <= cap) memcpy(out, sink.data, sink.size);
  free(sink.data);
  return size;
}
