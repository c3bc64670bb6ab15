/* jpeg_enc_ref.c -- TEST INFRASTRUCTURE: the compress side of the system's libjpeg (libjpeg.so.8 = libjpeg-turbo with the v8 ABI;
 * the image has the library but not its headers), driven the way cv::imencode(".jpg", img) of OpenCV 3.2 drives it
 * (modules/imgcodecs/src/grfmt_jpeg.cpp, JpegEncoder::write): jpeg_create_compress, a memory destination, image_width /
 * image_height, input_components 1 + JCS_GRAYSCALE or 3 + JCS_RGB, jpeg_set_defaults, jpeg_set_quality(quality, TRUE) (95 unless
 * the caller says otherwise; no progressive mode, no optimised tables, no restart interval), jpeg_start_compress(TRUE), one
 * jpeg_write_scanlines per row -- a 3-channel row is BGR in the Mat and goes through a BGR -> RGB copy first -- and
 * jpeg_finish_compress.  Bound by hand like jpeg_ref.c: the public prefix of struct jpeg_compress_struct up to in_color_space is
 * the same in every libjpeg since 6b; its total size is asked of the library (a deliberately wrong size makes
 * jpeg_CreateCompress report the right one), and the layout is checked by decoding what was written.
 *     gcc -O2 -shared -fPIC tests/cpp/jpeg_enc_ref.c -o <out>.so -l:libjpeg.so.8 */
#include <setjmp.h>
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

extern void* jpeg_std_error(void* err);
extern void jpeg_CreateCompress(void* cinfo, int version, size_t structsize);
extern void jpeg_destroy_compress(void* cinfo);
extern void jpeg_mem_dest(void* cinfo, unsigned char** outbuffer, unsigned long* outsize);
extern void jpeg_set_defaults(void* cinfo);
extern void jpeg_set_quality(void* cinfo, int quality, int force_baseline);
extern void jpeg_start_compress(void* cinfo, int write_all_tables);
extern unsigned int jpeg_write_scanlines(void* cinfo, unsigned char** rows, unsigned int num_lines);
extern void jpeg_finish_compress(void* cinfo);

enum { kImageWidth = 48, kImageHeight = 52, kInputComponents = 56, kInColorSpace = 60, kErrMsgCode = 40, kErrMsgParm = 44,
       kErrOutputMessage = 16 };

static jmp_buf jump;
static int last_code, probed_size;
static void on_error(void* cinfo) {
  char* err = *(char**)cinfo;
  last_code = *(int*)(err + kErrMsgCode);
  probed_size = *(int*)(err + kErrMsgParm);
  longjmp(jump, 1);
}
static void on_output(void* cinfo) { (void)cinfo; }  /* (no text on stderr) */

int jpeg_enc_ref_last_error_code(void) { return last_code; }

/* -> the file's size (its bytes in out[0 .. size), when size <= cap), 0: libjpeg refused, -1: bad arguments.  src: rows of
 * `pitch` bytes, `channels` (1: gray, 3: B G R) bytes per pixel. */
long jpeg_enc_ref(const unsigned char* src, int width, int height, int channels, size_t pitch, int quality, unsigned char* out,
                  size_t cap) {
  static char err[1024];
  static size_t struct_size;
  char* volatile cinfo = NULL;
  unsigned char* volatile row = NULL;
  unsigned char* mem = NULL;
  unsigned long mem_size = 0;
  if (!src || width < 1 || height < 1 || (channels != 1 && channels != 3) || pitch < (size_t)width * channels) return -1;
  last_code = 0;
  memset(err, 0, sizeof(err));
  jpeg_std_error(err);
  *(void**)err = (void*)on_error;
  *(void**)(err + kErrOutputMessage) = (void*)on_output;
  if (struct_size == 0) {  /* ask the library how large its struct is */
    char* probe = (char*)calloc(1, 8192);
    *(void**)probe = err;
    if (!setjmp(jump)) jpeg_CreateCompress(probe, 80, 12345);
    free(probe);
    if (probed_size < 400 || probed_size > 4096) return 0;
    struct_size = (size_t)probed_size;
  }
  cinfo = (char*)calloc(1, struct_size + 64);
  *(void**)cinfo = err;
  if (setjmp(jump)) {
    jpeg_destroy_compress(cinfo);
    free(cinfo);
    free(row);
    free(mem);
    return 0;
  }
  jpeg_CreateCompress(cinfo, 80, struct_size);
  jpeg_mem_dest(cinfo, &mem, &mem_size);
  *(unsigned int*)(cinfo + kImageWidth) = (unsigned int)width;
  *(unsigned int*)(cinfo + kImageHeight) = (unsigned int)height;
  *(int*)(cinfo + kInputComponents) = channels;
  *(int*)(cinfo + kInColorSpace) = channels == 1 ? 1 : 2; /* JCS_GRAYSCALE : JCS_RGB */
  jpeg_set_defaults(cinfo);
  jpeg_set_quality(cinfo, quality, 1);
  jpeg_start_compress(cinfo, 1);
  if (channels == 3) row = (unsigned char*)malloc((size_t)width * 3 + 64);
  for (int y = 0; y < height; y++) {
    const unsigned char* s = src + (size_t)y * pitch;
    unsigned char* rows[1];
    if (channels == 3) {
      for (int x = 0; x < width; x++) {  /* icvCvt_BGR2RGB_8u_C3R */
        row[3 * x] = s[3 * x + 2];
        row[3 * x + 1] = s[3 * x + 1];
        row[3 * x + 2] = s[3 * x];
      }
      rows[0] = row;
    } else {
      rows[0] = (unsigned char*)s;
    }
    jpeg_write_scanlines(cinfo, rows, 1);
  }
  jpeg_finish_compress(cinfo);
  const long size = (long)mem_size;
  if (out && mem_size <= cap) memcpy(out, mem, mem_size);
  jpeg_destroy_compress(cinfo);
  free(cinfo);
  free(row);
  free(mem);
  return size;
}
