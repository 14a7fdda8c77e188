/* htktext.h -- the one reader and the one writer of HTK's text conventions that the host files share (htktext.c). */
#ifndef HTKAMD_HTKTEXT_H
#define HTKAMD_HTKTEXT_H
#include <stddef.h>
#include <stdio.h>

typedef struct { const char *p, *end; int wasQuoted; } htx_src;        /* text still to read; wasQuoted: the last string stood in quotes */

/* what reading one string can come to */
enum { HTX_GOT = 1, HTX_NONE = 0, HTX_OPEN = -1, HTX_LONG = -2 };
#define HTX_LINE 1                            /* a newline ends the scan: it is not passed, and a quoted string may not hold one */

int htx_escaped(htx_src *s);                  /* the character after a backslash: itself, or three octal digits; -1 when it is not there */
int htx_read_string(htx_src *s, int flags, const char *stops, char *buf, size_t nb);
void htx_skip_line(htx_src *s);               /* past the next newline */
const char *htx_result_text(int r);           /* "a quoted string is not closed" / "a string is too long" */

/* ReWriteString: q = '\'' or '"' (always quoted), '\\' (never quoted, a leading quote escaped), 0 (quoted only when s starts with a quote).
   Like snprintf: returns the length of the whole result, which fits when that is below nd. */
#define HTX_ESCAPE '\\'
size_t htx_rewrite(const char *s, char q, char *dst, size_t nd);
int htx_write_string(FILE *f, const char *s, char q, int width);       /* as printf's %*s pads; -1: out of memory */

enum { HTX_EOPEN = 1, HTX_ENOMEM = 2 };
char *htx_read_file(const char *path, size_t *len, int *why);          /* NUL-terminated; NULL and *why on failure */

/* one line of an HMM list: a logical name and an optional physical one (*ph = 0 when absent); blank lines are passed over */
int htx_hmmlist_next(htx_src *s, char *lo, size_t nlo, char *ph, size_t nph);

/* one dictionary entry; the strings belong to the entry and live until the next call or htx_dict_free */
enum { HTX_OUT_ABSENT = 0, HTX_OUT_EMPTY, HTX_OUT_GIVEN };
typedef struct {
   char *word, *outSym; int outKind;
   int hasProb; float prob;                   /* as the reference keeps it: a float, 1.0 when none is given */
   int nPhones; char **phone;
   char *text; size_t capText, capPhones;     /* the entry's own storage */
} htx_dict_entry;
int htx_dict_next(htx_src *s, const char *path, htx_dict_entry *e);    /* HTX_GOT, HTX_NONE, or an HTKAMD_E* code with the error set */
void htx_dict_free(htx_dict_entry *e);

/* the fields of an SLF text */
enum { HTX_F_FIELD = 1, HTX_F_EOL = 0, HTX_F_EOF = -1, HTX_F_DOT = 2, HTX_F_ERR = -2 };
int htx_slf_next_field(htx_src *s, const char *path, char *name, size_t nn, char *val, size_t nv);
int htx_slf_number(const char *buf, double *out, int wantInt, const char *path, char field);

#endif
