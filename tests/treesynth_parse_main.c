/* A stand-alone driver for the trees-file reader (htkamd_mmf_load_trees, htk_amd/host/treesynth.c), built by tests/test_treesynth_host.py
 * from the host files alone under -fsanitize=address,undefined:
 *     treesynth_parse_main <model set> <hmm list> <trees file> ...
 * loads the set once, then every trees file into it (the held trees are saved again after a file that was taken), and prints one line per
 * file: "<rc> <file>: <reason>".  The exit status is 0 when every file was either taken or refused; anything the sanitizers find ends it. */
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include "htk_amd.h"

static char g_err[1024];
void htkamd_set_error(const char *fmt, ...) { va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof g_err, fmt, ap); va_end(ap); }
const char *htkamd_last_error(void) { return g_err; }

int main(int argc, char **argv)
{
   if (argc < 4) { fprintf(stderr, "usage: %s mmf list trees...\n", argv[0]); return 2; }
   for (int k = 3; k < argc; k++) {
      htkamd_mmf *s = NULL;
      if (htkamd_mmf_create(&s) || htkamd_mmf_read(s, argv[1], NULL) || htkamd_mmf_finish(s, argv[2], NULL, NULL)) { fprintf(stderr, "cannot load the set: %s\n", g_err); return 2; }
      g_err[0] = 0;
      const int rc = htkamd_mmf_load_trees(s, argv[k]);
      printf("%d %s: %s\n", rc, argv[k], rc ? g_err : "taken");
      if (!rc) {
         char out[1200];
         snprintf(out, sizeof(out), "%s.saved", argv[k]);
         if (htkamd_mmf_save_trees(s, out)) { fprintf(stderr, "cannot save the trees of %s: %s\n", argv[k], g_err); return 2; }
      } else if (!g_err[0]) { fprintf(stderr, "%s was refused without a reason\n", argv[k]); return 2; }
      htkamd_mmf_destroy(s);
   }
   return 0;
}
