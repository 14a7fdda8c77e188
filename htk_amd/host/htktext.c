/* htktext.c -- HTK's text conventions, stated once for every host file that reads or writes them:
 *   ReadString (HShell.c:1159) over a span of memory, with the extra terminators of ParseAlpha (HHEd.c:381) and GetAlpha (HUtil.c:660);
 *   ReWriteString / WriteString (HShell.c:1268-1341);
 *   a whole text file in one buffer;
 *   one line of an HMM list (MakeHMMSet), one entry of a dictionary (ReadDictWord HDict.c:224);
 *   GetNextFieldName / GetFieldValue / ParseNumber of the SLF reader (HNet.c:707-800), with the reference's refusals.
 * Pure C: no device, and of the library only its error call and codes.
 */
#include <ctype.h>
#include <stdlib.h>
#include <string.h>
#include "../csrc/internal.h"
#include "htktext.h"

static int is_octal(int c) { return c >= '0' && c <= '7'; }

/* s->p stands behind a backslash.  Any character stands for itself; an octal digit must be the first of three.  What the reference has
   read when it gives up (the end of the text, or a digit that is none) is read here too. */
int htx_escaped(htx_src *s)
{
   if (s->p >= s->end) return -1;
   int c = (unsigned char)*s->p++;
   if (!is_octal(c)) return c;
   int n = c - '0';
   for (int k = 0; k < 2; k++) {
      if (s->p >= s->end) return -1;
      c = (unsigned char)*s->p++;
      if (!is_octal(c)) return -1;
      n = n * 8 + c - '0';
   }
   return n & 255;
}

/* HTX_NONE is also what a broken escape gives (the reference's ReadString returns FALSE for both) */
int htx_read_string(htx_src *s, int flags, const char *stops, char *buf, size_t nb)
{
   const int line = flags & HTX_LINE;
   size_t n = 0;
   s->wasQuoted = 0;
   while (s->p < s->end && isspace((unsigned char)*s->p) && !(line && *s->p == '\n')) s->p++;
   if (s->p >= s->end || *s->p == '\n') return HTX_NONE;
   char q = 0;
   if (*s->p == '"' || *s->p == '\'') { q = *s->p++; s->wasQuoted = 1; }
   for (;;) {
      int c = s->p < s->end ? (unsigned char)*s->p : -1;
      if (q) {
         if (c < 0 || (line && c == '\n')) return HTX_OPEN;
         if (c == q) { s->p++; break; }
      } else if (c < 0 || isspace(c) || (stops && c && strchr(stops, c))) break;
      s->p++;
      if (c == '\\' && (c = htx_escaped(s)) < 0) return HTX_NONE;
      if (n + 1 >= nb) return HTX_LONG;
      buf[n++] = (char)c;
   }
   buf[n] = 0;
   return HTX_GOT;
}

void htx_skip_line(htx_src *s)
{
   while (s->p < s->end && *s->p != '\n') s->p++;
   if (s->p < s->end) s->p++;
}

const char *htx_result_text(int r)
{
   return r == HTX_OPEN ? "ReadString: File end within quoted string (5013)" : (r == HTX_LONG ? "ReadString: String too long (5013)" : "string expected");
}

size_t htx_rewrite(const char *s, char q, char *dst, size_t nd)
{
   size_t n = 0;
#define PUT(c) do { if (n + 1 < nd) dst[n] = (char)(c); n++; } while (0)
   if (q != '\\' && q != '\'' && q != '"') q = (char)(s[0] == '"' ? '\'' : (s[0] == '\'' ? '"' : 0));
   if (q && q != '\\') PUT(q);
   for (const unsigned char *p = (const unsigned char *)s; *p; p++) {
      if (*p == '\\' || *p == (unsigned char)q || (q == '\\' && p == (const unsigned char *)s && (*p == '\'' || *p == '"'))) { PUT('\\'); PUT(*p); }
      else if (*p >= 32 && *p < 127) PUT(*p);                /* isprint in the C locale */
      else { PUT('\\'); PUT(((*p / 64) % 8) + '0'); PUT(((*p / 8) % 8) + '0'); PUT((*p % 8) + '0'); }
   }
   if (q && q != '\\') PUT(q);
#undef PUT
   if (nd) dst[n < nd ? n : nd - 1] = 0;
   return n;
}

int htx_write_string(FILE *f, const char *s, char q, int width)
{
   char small[256], *b = small;
   const size_t n = htx_rewrite(s, q, small, sizeof(small));
   if (n >= sizeof(small)) {
      if (!(b = (char *)malloc(n + 1))) return -1;
      htx_rewrite(s, q, b, n + 1);
   }
   fprintf(f, "%*s", width, b);
   if (b != small) free(b);
   return 0;
}

char *htx_read_file(const char *path, size_t *len, int *why)
{
   FILE *f = fopen(path, "rb");
   *len = 0;
   if (!f) { *why = HTX_EOPEN; return NULL; }
   size_t cap = 1 << 16, n = 0;
   char *b = (char *)malloc(cap + 1);
   while (b) {
      const size_t got = fread(b + n, 1, cap - n, f);
      n += got;
      if (got == 0) break;
      if (n == cap) { char *nb = (char *)realloc(b, 2 * cap + 1); if (!nb) { free(b); b = NULL; break; } b = nb; cap *= 2; }
   }
   fclose(f);
   if (!b) { *why = HTX_ENOMEM; return NULL; }
   b[n] = 0; *len = n;
   return b;
}

int htx_hmmlist_next(htx_src *s, char *lo, size_t nlo, char *ph, size_t nph)
{
   int r = htx_read_string(s, 0, NULL, lo, nlo);             /* over blank lines */
   if (r != HTX_GOT) return r;
   r = htx_read_string(s, HTX_LINE, NULL, ph, nph);
   if (r < 0) return r;
   if (r == HTX_NONE) ph[0] = 0;
   htx_skip_line(s);
   return HTX_GOT;
}

void htx_dict_free(htx_dict_entry *e) { free(e->text); free(e->phone); memset(e, 0, sizeof(*e)); }

int htx_dict_next(htx_src *s, const char *path, htx_dict_entry *e)
{
   while (s->p < s->end && isspace((unsigned char)*s->p)) s->p++;
   if (s->p >= s->end) return HTX_NONE;
   /* a string is never longer than its text, so the line's length bounds the entry's storage */
   const char *eol = (const char *)memchr(s->p, '\n', (size_t)(s->end - s->p));
   const size_t L = (size_t)((eol ? eol : s->end) - s->p) + 2;
   if (L > e->capText) { char *t = (char *)realloc(e->text, L); if (!t) goto nomem; e->text = t; e->capText = L; }
   if (L / 2 + 1 > e->capPhones) { char **ph = (char **)realloc(e->phone, sizeof(char *) * (L / 2 + 1)); if (!ph) goto nomem; e->phone = ph; e->capPhones = L / 2 + 1; }
   char *at = e->text, *const top = e->text + e->capText;
   e->word = at; e->outSym = NULL; e->outKind = HTX_OUT_ABSENT; e->hasProb = 0; e->prob = 1.0f; e->nPhones = 0;
   int r = htx_read_string(s, HTX_LINE, NULL, at, (size_t)(top - at));
   for (int first = 1; r == HTX_GOT; first = 0, r = htx_read_string(s, HTX_LINE, NULL, at, (size_t)(top - at))) {
      const size_t n = strlen(at);
      char *tok = at, *stop = at;
      at += n + 1;
      if (first) continue;
      if (n && tok[0] == '[' && tok[n - 1] == ']') {
         if (e->outKind != HTX_OUT_ABSENT || e->nPhones) { htkamd_set_error("%s: ReadDict: Only single outsym allowed for word %s (8050)", path, e->word); return HTKAMD_EMODEL; }
         tok[n - 1] = 0; e->outSym = tok + 1;
         e->outKind = tok[1] ? HTX_OUT_GIVEN : HTX_OUT_EMPTY;
         continue;
      }
      float v = 0.0f;
      if (e->nPhones == 0 && !e->hasProb) v = (float)strtod(tok, &stop);
      if (stop != tok) {
         if (v <= 0.0 || v > 1.0 || *stop) { htkamd_set_error("%s: ReadDict: Probability malformed %s (8050)", path, tok); return HTKAMD_EMODEL; }
         e->hasProb = 1; e->prob = v;
      } else e->phone[e->nPhones++] = tok;
   }
   if (r < 0) { htkamd_set_error("%s: ReadDict: word %s: %s", path, e->word, htx_result_text(r)); return HTKAMD_EMODEL; }
   if (s->p < s->end && *s->p != '\n') { htkamd_set_error("%s: ReadDict: Phone or outsym expected in word %s (8050)", path, e->word); return HTKAMD_EMODEL; }
   return HTX_GOT;
nomem:
   htkamd_set_error("%s: ReadDict: out of memory", path);
   return HTKAMD_ENOMEM;
}

/* GetNextFieldName + GetFieldValue (HNet.c:707-767) */
int htx_slf_next_field(htx_src *s, const char *path, char *name, size_t nn, char *val, size_t nv)
{
   while (s->p < s->end && isspace((unsigned char)*s->p) && *s->p != '\n') s->p++;
   if (s->p >= s->end) return HTX_F_EOF;
   if (*s->p == '\n') { s->p++; return HTX_F_EOL; }
   if (*s->p == '.') { s->p++; return HTX_F_DOT; }
   if (!isalnum((unsigned char)*s->p)) {
      if (*s->p != '#') { htkamd_set_error("%s: GetNextFieldName: Field name expected (8250)", path); return HTX_F_ERR; }
      htx_skip_line(s);
      return HTX_F_EOL;
   }
   size_t n = 0;
   while (s->p < s->end && isalnum((unsigned char)*s->p)) { if (n + 1 < nn) name[n++] = *s->p; s->p++; }
   name[n] = 0;
   if (s->p >= s->end) { htkamd_set_error("%s: GetNextFieldName: EOF whilst reading field name (8250)", path); return HTX_F_ERR; }
   if (*s->p == '~') { htkamd_set_error("%s: field %s is binary (~): binary lattices are not supported", path, name); return HTX_F_ERR; }
   if (*s->p != '=') { htkamd_set_error("%s: GetNextFieldName: Field delimiter expected %s|%c| (8250)", path, name, *s->p); return HTX_F_ERR; }
   s->p++;
   if (s->p >= s->end || isspace((unsigned char)*s->p)) { htkamd_set_error("%s: GetFieldValue: Field value expected (8250)", path); return HTX_F_ERR; }
   const int r = htx_read_string(s, HTX_LINE, NULL, val, nv);
   if (r < 0) { htkamd_set_error("%s: field %s: %s", path, name, htx_result_text(r)); return HTX_F_ERR; }
   if (r == HTX_NONE) val[0] = 0;
   return HTX_F_FIELD;
}

/* ParseNumber (HNet.c:770) */
int htx_slf_number(const char *buf, double *out, int wantInt, const char *path, char field)
{
   char *e;
   if (!(isdigit((unsigned char)buf[0]) || ((buf[0] == '-' || buf[0] == '+') && isdigit((unsigned char)buf[1])))) {
      htkamd_set_error("%s: %s: %c field expects numeric value (%s) (8250)", path, wantInt ? "GetIntField" : "GetFltField", field, buf);
      return HTKAMD_EMODEL;
   }
   *out = strtod(buf, &e);
   if (wantInt && !(*out >= -2147483647.0 && *out <= 2147483647.0)) { htkamd_set_error("%s: GetIntField: %c field value out of range (%s) (8250)", path, field, buf); return HTKAMD_EMODEL; }
   if (wantInt && strchr(buf, '.')) { htkamd_set_error("%s: GetIntField: %c field expects integer value (%s) (8250)", path, field, buf); return HTKAMD_EMODEL; }
   return HTKAMD_OK;
}
