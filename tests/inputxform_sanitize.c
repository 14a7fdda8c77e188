/* inputxform_sanitize.c -- stand-alone driver (TEST INFRASTRUCTURE) for the host C that reads and writes input transforms, meant to be
 * built with -fsanitize=address,undefined together with htk_amd/host/mmf.c and the host files it calls (tests/test_inputxform_host.py
 * does that).
 *
 *    inputxform_sanitize <scratch dir> <hmm list> <file> ...
 *
 * Every file is read whole -- a name that ends in ".mmf" as a model set (htkamd_mmf_read + htkamd_mmf_finish, then written back as text
 * and as binary and both read again), any other as a transform file (htkamd_inputxform_read, written as text and as binary, both read
 * again and compared with the first) -- and then as truncated copies: cut at every 41st byte and at each of its last 48 bytes, where the
 * readers may refuse but must neither read outside their buffers nor leak into undefined behaviour.
 * Prints "OK <files> <truncated copies>" and returns 0 when every whole file was served.
 */
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../htk_amd/csrc/internal.h"

static char g_err[2048];
void htkamd_set_error(const char *fmt, ...) { va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof g_err, fmt, ap); va_end(ap); }
const char *htkamd_last_error(void) { return g_err; }

static const char *g_list;

static int is_set(const char *path) { const size_t n = strlen(path); return n > 4 && !strcmp(path + n - 4, ".mmf"); }

static int same_xform(const htkamd_inputxform *a, const htkamd_inputxform *b)
{
   int na, nb;
   const float *ba = htkamd_inputxform_bias(a, &na), *bb = htkamd_inputxform_bias(b, &nb);
   const int r = htkamd_inputxform_rows(a), c = htkamd_inputxform_cols(a);
   return !strcmp(htkamd_inputxform_name(a), htkamd_inputxform_name(b)) && !strcmp(htkamd_inputxform_mask(a), htkamd_inputxform_mask(b)) &&
          !strcmp(htkamd_inputxform_parm_kind(a), htkamd_inputxform_parm_kind(b)) && htkamd_inputxform_prequal(a) == htkamd_inputxform_prequal(b) &&
          r == htkamd_inputxform_rows(b) && c == htkamd_inputxform_cols(b) && htkamd_inputxform_vec_size(a) == htkamd_inputxform_vec_size(b) &&
          !memcmp(htkamd_inputxform_matrix(a), htkamd_inputxform_matrix(b), sizeof(float) * (size_t)r * (size_t)c) &&
          na == nb && (na == 0 || !memcmp(ba, bb, sizeof(float) * (size_t)na)) && htkamd_inputxform_logdet(a) == htkamd_inputxform_logdet(b);
}

/* one model file: 0 = served */
static int read_set(const char *path, const char *scratch, int rewrite)
{
   htkamd_mmf *s;
   char out[2][2048];
   int rc;
   if (htkamd_mmf_create(&s)) return 1;
   rc = htkamd_mmf_read(s, path, NULL);
   if (!rc) rc = htkamd_mmf_finish(s, g_list, NULL, NULL);
   if (!rc && rewrite) {
      const htkamd_model_desc *d = htkamd_mmf_desc(s);
      for (int b = 0; b < 2 && !rc; b++) {
         snprintf(out[b], sizeof(out[b]), "%s/rewritten%d.mmf", scratch, b);
         rc = b ? htkamd_mmf_write_binary(s, d->mean, d->var, d->gconst, d->compWeight, d->transP, out[b], NULL)
                : htkamd_mmf_write(s, d->mean, d->var, d->gconst, d->compWeight, d->transP, out[b], NULL);
      }
      for (int b = 0; b < 2 && !rc; b++) {
         htkamd_mmf *t;
         if (htkamd_mmf_create(&t)) { rc = 1; break; }
         rc = htkamd_mmf_read(t, out[b], NULL);
         if (!rc) rc = htkamd_mmf_finish(t, g_list, NULL, NULL);
         if (!rc && (!htkamd_mmf_inputxform(s) != !htkamd_mmf_inputxform(t) ||
                     (htkamd_mmf_inputxform(s) && memcmp(htkamd_inputxform_matrix(htkamd_mmf_inputxform(s)), htkamd_inputxform_matrix(htkamd_mmf_inputxform(t)),
                                                         sizeof(float) * (size_t)htkamd_inputxform_rows(htkamd_mmf_inputxform(s)) * (size_t)htkamd_inputxform_cols(htkamd_mmf_inputxform(s)))))) {
            htkamd_set_error("%s: the transform changed on the way through the writer", out[b]); rc = 1;
         }
         htkamd_mmf_destroy(t);
      }
   }
   htkamd_mmf_destroy(s);
   return rc;
}

static int read_xform(const char *path, const char *scratch, int rewrite)
{
   htkamd_inputxform *x = NULL;
   int rc = htkamd_inputxform_read(path, &x);
   for (int b = 0; b < 2 && !rc && rewrite; b++) {
      char out[2048];
      htkamd_inputxform *y = NULL;
      snprintf(out, sizeof(out), "%s/rewritten%d.xf", scratch, b);
      rc = htkamd_inputxform_write(x, out, b);
      if (!rc) rc = htkamd_inputxform_read(out, &y);
      if (!rc && !same_xform(x, y)) { htkamd_set_error("%s: the transform changed on the way through the writer", out); rc = 1; }
      htkamd_inputxform_free(y);
   }
   htkamd_inputxform_free(x);
   return rc;
}

int main(int argc, char **argv)
{
   int nFiles = 0, nCut = 0;
   if (argc < 4) { fprintf(stderr, "usage: inputxform_sanitize scratch hmmlist file ...\n"); return 2; }
   g_list = argv[2];
   for (int a = 3; a < argc; a++) {
      const char *path = argv[a];
      const int set = is_set(path);
      if (set ? read_set(path, argv[1], 1) : read_xform(path, argv[1], 1)) { fprintf(stderr, "%s: %s\n", path, g_err); return 1; }
      nFiles++;
      FILE *f = fopen(path, "rb");
      if (!f) { fprintf(stderr, "%s: cannot open\n", path); return 1; }
      fseek(f, 0, SEEK_END);
      const long len = ftell(f);
      fseek(f, 0, SEEK_SET);
      unsigned char *buf = (unsigned char *)malloc((size_t)len + 1);
      if (fread(buf, 1, (size_t)len, f) != (size_t)len) { fprintf(stderr, "%s: short read\n", path); return 1; }
      fclose(f);
      for (long cut = 0; cut < len; cut += (cut + 48 >= len) ? 1 : 41) {
         char tmp[2048];
         snprintf(tmp, sizeof(tmp), "%s/%s", argv[1], set ? "cut.mmf" : "cut.xf");
         FILE *g = fopen(tmp, "wb");
         if (!g) { fprintf(stderr, "%s: cannot create\n", tmp); return 1; }
         fwrite(buf, 1, (size_t)cut, g);
         fclose(g);
         (void)(set ? read_set(tmp, argv[1], 0) : read_xform(tmp, argv[1], 0));      /* may refuse; must not misbehave */
         nCut++;
      }
      free(buf);
   }
   printf("OK %d %d\n", nFiles, nCut);
   return 0;
}
