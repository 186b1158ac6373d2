// tsa -- score one triple on the GPU and print the testbench's line
// "TriAlign Score: <n>" (src/TriAlign_tb.sv:339-341).
//   tsa A.dat B.dat C.dat [--kernel auto|plane|pencil] [--device N]
//       [--s3 rtl|sop] [--bits B] [--match M --mismatch X --go O --ge E]
//       [--states] [--align [--end corner|face|any] [--grid]] [--score-end face|any [--kernel plane|auto | --lap]]
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../include/trialign.h"
#include "seqio.h"

static int usage() {
  fprintf(stderr,
          "usage: tsa A B C [--kernel auto|plane|pencil] [--device N] [--s3 rtl|sop]\n"
          "           [--bits B] [--match M] [--mismatch X] [--go O] [--ge E] [--states]\n"
          "           [--align]   (also print the optimal alignment; tsa_align_gpu)\n"
          "           [--end corner|face|any]   (with --align: where the path may end; face and any\n"
          "                                      go through tsa_align_batch_ends and print the end)\n"
          "           [--grid]   (with --align: the grid path, for cubes whose pointers do not fit memory;\n"
          "                       tsa_align_batch_grid, or tsa_align_batch_grid_ends with --end face|any)\n"
          "           [--score-end face|any]   (without --align: the end-free score and its end cell,\n"
          "                                     tsa_score_batch_ends; no alignment is traced. Its plan is\n"
          "                                     the factored helix; --kernel plane runs the end search of the\n"
          "                                     literal helix instead (any parameter set), --kernel auto the\n"
          "                                     factored one where it admits the request and the literal one\n"
          "                                     otherwise (tsa_score_batch_ends_ex). With --kernel pencil or\n"
          "                                     --states a usage error)\n"
          "           [--lap]   (with --score-end: the end search of the checked lap kernel, for cubes beyond\n"
          "                      the helix forms (max_lc > 256), tsa_score_batch_ends_lap; with --kernel a\n"
          "                      usage error)\n"
          "A/B/C: dat files (one symbol 0..4 per line) or FASTA (A=0 T=1 C=2 G=3 N=4)\n");
  return 2;
}

int main(int argc, char **argv) {
  const char *files[3];
  int nf = 0, device = 0, kernel = TSA_KERNEL_AUTO, kernel_set = 0, states = 0, align = 0, grid = 0, end = TSA_END_CORNER, score_end = TSA_END_CORNER, lap = 0;
  tsa_params p;
  tsa_default_params(&p);
  for (int i = 1; i < argc; ++i) {
    const char *a = argv[i];
    auto next = [&](void) -> const char * { return (i + 1 < argc) ? argv[++i] : nullptr; };
    if (!strcmp(a, "--kernel")) {
      const char *v = next();
      if (!v) return usage();
      kernel_set = 1;
      kernel = !strcmp(v, "plane") ? TSA_KERNEL_PLANE : !strcmp(v, "pencil") ? TSA_KERNEL_PENCIL : TSA_KERNEL_AUTO;
    } else if (!strcmp(a, "--device")) { const char *v = next(); if (!v) return usage(); device = atoi(v); }
    else if (!strcmp(a, "--s3")) { const char *v = next(); if (!v) return usage(); p.s3_mode = !strcmp(v, "sop") ? TSA_S3_SOP : TSA_S3_RTL; }
    else if (!strcmp(a, "--bits")) { const char *v = next(); if (!v) return usage(); p.score_bits = atoi(v); }
    else if (!strcmp(a, "--match")) { const char *v = next(); if (!v) return usage(); p.match = atoi(v); }
    else if (!strcmp(a, "--mismatch")) { const char *v = next(); if (!v) return usage(); p.mismatch = atoi(v); }
    else if (!strcmp(a, "--go")) { const char *v = next(); if (!v) return usage(); p.gap_open = atoi(v); }
    else if (!strcmp(a, "--ge")) { const char *v = next(); if (!v) return usage(); p.gap_extend = atoi(v); }
    else if (!strcmp(a, "--states")) states = 1;
    else if (!strcmp(a, "--align")) align = 1;
    else if (!strcmp(a, "--grid")) grid = 1;
    else if (!strcmp(a, "--lap")) lap = 1;
    else if (!strcmp(a, "--end")) {
      const char *v = next();
      if (!v) return usage();
      if (!strcmp(v, "corner")) end = TSA_END_CORNER;
      else if (!strcmp(v, "face")) end = TSA_END_FACE;
      else if (!strcmp(v, "any")) end = TSA_END_ANY;
      else return usage();
    }
    else if (!strcmp(a, "--score-end")) {
      const char *v = next();
      if (!v) return usage();
      if (!strcmp(v, "face")) score_end = TSA_END_FACE;
      else if (!strcmp(v, "any")) score_end = TSA_END_ANY;
      else return usage();
    }
    else if (a[0] == '-' && a[1] == '-') return usage();
    else if (nf < 3) files[nf++] = a;
    else return usage();
  }
  if (nf != 3 || ((end != TSA_END_CORNER || grid) && !align)) return usage();
  if (score_end != TSA_END_CORNER && (align || states || (kernel_set && kernel == TSA_KERNEL_PENCIL))) return usage();
  if (lap && (score_end == TSA_END_CORNER || kernel_set)) return usage();
  uint8_t *s[3];
  int64_t n[3];
  for (int k = 0; k < 3; ++k) {
    n[k] = tsa_read_sequence(files[k], &s[k]);
    if (n[k] < 0) { fprintf(stderr, "tsa: cannot read %s\n", files[k]); return 1; }
  }
  int32_t score = 0, fin[7];
  if (score_end != TSA_END_CORNER) {  // a batch of one: the three sequences back to back
    const int64_t cap = n[0] + n[1] + n[2];
    uint8_t *seqs = (uint8_t *)malloc((size_t)cap);
    const int64_t off[4] = {0, n[0], n[0] + n[1], cap};
    int32_t en[3] = {0, 0, 0};
    if (seqs)
      for (int k = 0; k < 3; ++k) memcpy(seqs + off[k], s[k], (size_t)n[k]);
    const int rc = !seqs ? TSA_ENOMEM
                   : lap      ? tsa_score_batch_ends_lap(seqs, off, 1, &p, score_end, &score, en, device)
                   : kernel_set ? tsa_score_batch_ends_ex(seqs, off, 1, &p, score_end, kernel, &score, en, device)
                                : tsa_score_batch_ends(seqs, off, 1, &p, score_end, &score, en, device);
    free(seqs);
    if (rc) { fprintf(stderr, "tsa: %s (%d)\n", tsa_strerror(rc), rc); return 1; }
    printf("TriAlign Score:        \t%d\n", score);
    printf("end (x1,y1,z1) = (%d,%d,%d)\n", en[0], en[1], en[2]);
    return 0;
  }
  int rc = tsa_score_gpu_ex(s[0], (int32_t)n[0], s[1], (int32_t)n[1], s[2], (int32_t)n[2], &p,
                            states ? TSA_KERNEL_PLANE : kernel, &score, states ? fin : nullptr, device);
  if (rc) { fprintf(stderr, "tsa: %s (%d)\n", tsa_strerror(rc), rc); return 1; }
  printf("TriAlign Score:        \t%d\n", score);
  if (states)
    printf("final states {M,Ix,Iy,Iz,Ixy,Iyz,Ixz}: %d %d %d %d %d %d %d\n", fin[0], fin[1], fin[2],
           fin[3], fin[4], fin[5], fin[6]);
  if (align) {
    const int64_t cap = n[0] + n[1] + n[2];
    uint8_t *mv = (uint8_t *)malloc((size_t)cap);
    int32_t nm = 0, st[3], en[3], sc = 0;
    if (!mv) rc = TSA_ENOMEM;
    else if (end == TSA_END_CORNER && !grid)
      rc = tsa_align_gpu(s[0], (int32_t)n[0], s[1], (int32_t)n[1], s[2], (int32_t)n[2], &p, &sc, mv, (int32_t)cap, &nm,
                         st, device);
    else {  // a batch of one: the three sequences back to back
      uint8_t *seqs = (uint8_t *)malloc((size_t)cap);
      const int64_t off[4] = {0, n[0], n[0] + n[1], cap};
      if (seqs)
        for (int k = 0; k < 3; ++k) memcpy(seqs + off[k], s[k], (size_t)n[k]);
      rc = !seqs                   ? TSA_ENOMEM
           : !grid                 ? tsa_align_batch_ends(seqs, off, 1, &p, end, &sc, mv, &nm, st, en, device)
           : end != TSA_END_CORNER ? tsa_align_batch_grid_ends(seqs, off, 1, &p, end, &sc, mv, &nm, st, en, device)
                                   : tsa_align_batch_grid(seqs, off, 1, &p, &sc, mv, &nm, st, device);
      free(seqs);
    }
    if (rc) { fprintf(stderr, "tsa: %s (%d)\n", tsa_strerror(rc), rc); free(mv); return 1; }
    static const int use[7][3] = {{1, 1, 1}, {1, 0, 0}, {0, 1, 0}, {0, 0, 1}, {1, 1, 0}, {0, 1, 1}, {1, 0, 1}};
    static const char *letters = "ATCGN";
    printf("alignment start (x0,y0,z0) = (%d,%d,%d), %d columns\n", st[0], st[1], st[2], nm);
    if (end != TSA_END_CORNER)
      printf("alignment end (x1,y1,z1) = (%d,%d,%d), score %d\n", en[0], en[1], en[2], sc);
    for (int k = 0; k < 3; ++k) {
      int64_t pos = st[k];
      putchar("ABC"[k]);
      putchar(' ');
      for (int32_t j = 0; j < nm; ++j) putchar(use[mv[j]][k] ? letters[s[k][pos++]] : '-');
      putchar('\n');
    }
    free(mv);
  }
  return 0;
}
