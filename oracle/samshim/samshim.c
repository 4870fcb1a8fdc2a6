/* oracle/samshim/samshim.c -- TEST INFRASTRUCTURE ONLY (never linked into the product).
 *
 * The reference checkout's samtools/ submodule is empty, so its dwgsim_eval cannot be built as it stands. dwgsim_eval.c needs little of
 * samtools: samopen / samread / samwrite / samclose, bam_init1 / bam_destroy1, bam_aux_get / bam_aux2i, a few accessor macros and three
 * structs. This file and samtools/{bam,sam}.h give exactly that, written from the SAM/BAM specification, so that the UNMODIFIED
 * dwgsim_eval.c compiles, links (with -lz -lm) and runs: oracle/_ref/dwgsim_eval, the anchor of tests/golden/eval_reference_runs.json.
 * It is linked in; it is no preload library.
 *
 * Text mode ("r", dwgsim_eval -S): header lines start with '@'; the SN: value of every @SQ line is a target; the header text is kept for -p.
 *   A record: QNAME; FLAG by strtol(.., 0, 0); tid by looking RNAME up among the targets (-1 otherwise); pos = atoi(POS) - 1; MAPQ by atoi;
 *   the CIGAR packed as len << 4 | op; no sequence or qualities are stored (l_qseq 0: dwgsim_eval.c never reads them); the optional fields as
 *   BAM aux bytes: an `i` value takes the smallest of c C s S i I that holds it (low 32 bits of anything wider), A f Z H are kept, a B array
 *   is stored as sub-type, count, values, so that it can be walked.
 * Binary mode ("rb"): zlib's gzread over the BGZF members: magic, header text, the reference list (the targets), then records: core is
 *   unpacked from the 32 fixed bytes, data is the rest of the record, untouched.
 * bam_aux_get walks real aux bytes (B arrays included); bam_aux2i gives c C s S i I as int32_t and 0 for any other type.
 * samwrite prints the line as it was read (text mode) or a fixed placeholder (BAM): the record text of -p is a documented difference of the
 *   product and is never compared.
 *
 * NOT restated: samtools' handling of malformed input (lines with fewer than 11 fields, bad CIGAR operators, aux fields of unknown type or
 * cut short, names longer than 254 bytes, a damaged or truncated BAM container: here the read just ends), its "[samopen] SAM header is
 * present" and other diagnostics on stderr, the -t / fn_list ways to supply targets, its re-serialisation of records on output, CRAM, the
 * index, and everything else of samtools that dwgsim_eval.c does not call. Cases are recorded only on input that avoids all of it. */
#include <ctype.h>
#include <zlib.h>
#include "samtools/sam.h"

bam1_t *bam_init1(void) { return (bam1_t*)calloc(1, sizeof(bam1_t)); }

void bam_destroy1(bam1_t *b)
{
  if (b == NULL) return;
  free(b->data); free(b->line); free(b);
}

static void header_destroy(bam_header_t *h)
{
  int32_t i;
  if (h == NULL) return;
  for (i = 0; i < h->n_targets; i++) free(h->target_name[i]);
  free(h->target_name); free(h->text); free(h);
}

static void header_add_target(bam_header_t *h, const char *name, size_t len)
{
  h->target_name = (char**)realloc(h->target_name, sizeof(char*) * (h->n_targets + 1));
  h->target_name[h->n_targets] = (char*)malloc(len + 1);
  memcpy(h->target_name[h->n_targets], name, len);
  h->target_name[h->n_targets++][len] = '\0';
}

/* ---- text mode ---- */

static void text_header_read(samfile_t *fp)
{
  bam_header_t *h = fp->header;
  int c;
  while ((c = getc(fp->fp)) == '@') {
    char *line = NULL; size_t cap = 0;
    ssize_t n = getline(&line, &cap, fp->fp);
    if (n < 0) n = 0;
    h->text = (char*)realloc(h->text, h->l_text + n + 2);
    h->text[h->l_text++] = '@';
    memcpy(h->text + h->l_text, line, n); h->l_text += n; h->text[h->l_text] = '\0';
    if (n >= 2 && line[0] == 'S' && line[1] == 'Q') {
      char *p = line;
      while ((p = strchr(p, '\t')) != NULL) {
        p++;
        if (0 == strncmp(p, "SN:", 3)) { header_add_target(h, p + 3, strcspn(p + 3, "\t\n")); break; }
      }
    }
    free(line);
  }
  if (c != EOF) ungetc(c, fp->fp);
}

typedef struct { uint8_t *s; size_t l, m; } buf_t;

static void put(buf_t *b, const void *p, size_t n)
{
  if (b->l + n > b->m) { b->m = (b->l + n) * 2 + 64; b->s = (uint8_t*)realloc(b->s, b->m); }
  memcpy(b->s + b->l, p, n); b->l += n;
}

static void put_int(buf_t *b, long long v)
{
  char t; int8_t c; uint8_t C; int16_t s; uint16_t S; int32_t i; uint32_t I;
  if (v < 0) {
    if (v >= INT8_MIN) { t = 'c'; c = (int8_t)v; put(b, &t, 1); put(b, &c, 1); }
    else if (v >= INT16_MIN) { t = 's'; s = (int16_t)v; put(b, &t, 1); put(b, &s, 2); }
    else { t = 'i'; i = (int32_t)(uint32_t)(unsigned long long)v; put(b, &t, 1); put(b, &i, 4); }
  } else {
    if (v <= UINT8_MAX) { t = 'C'; C = (uint8_t)v; put(b, &t, 1); put(b, &C, 1); }
    else if (v <= UINT16_MAX) { t = 'S'; S = (uint16_t)v; put(b, &t, 1); put(b, &S, 2); }
    else { t = 'I'; I = (uint32_t)(unsigned long long)v; put(b, &t, 1); put(b, &I, 4); }
  }
}

static size_t b_size(int sub)
{
  switch (sub) { case 'c': case 'C': return 1; case 's': case 'S': return 2; case 'i': case 'I': case 'f': return 4; }
  return 0;
}

static void put_aux(buf_t *b, const char *f)
{
  size_t n = strlen(f);
  if (n < 5 || f[2] != ':' || f[4] != ':') return;
  const char *v = f + 5; char ty = f[3];
  if (ty == 'i') { put(b, f, 2); put_int(b, strtoll(v, NULL, 10)); }
  else if (ty == 'A') { put(b, f, 2); put(b, "A", 1); put(b, v, 1); }
  else if (ty == 'f') { float x = strtof(v, NULL); put(b, f, 2); put(b, "f", 1); put(b, &x, 4); }
  else if (ty == 'Z' || ty == 'H') { put(b, f, 2); put(b, &ty, 1); put(b, v, strlen(v) + 1); }
  else if (ty == 'B' && b_size(v[0])) {
    char sub = v[0]; uint32_t cnt = 0; const char *p;
    for (p = v + 1; *p; p++) cnt += (*p == ',');
    put(b, f, 2); put(b, "B", 1); put(b, &sub, 1); put(b, &cnt, 4);
    for (p = v + 1; *p == ','; ) {
      char *e;
      if (sub == 'f') { float x = strtof(p + 1, &e); put(b, &x, 4); }
      else { long long x = strtoll(p + 1, &e, 10); put(b, &x, b_size(sub)); }      /* little-endian host: the low bytes */
      p = e;
    }
  }
}

static int text_read(samfile_t *fp, bam1_t *b)
{
  char *line = NULL, *f[12], *p; size_t cap = 0; int nf = 0, k;
  ssize_t n = getline(&line, &cap, fp->fp);
  buf_t d = {0, 0, 0};
  if (n <= 0) { free(line); return -1; }
  if (line[n - 1] == '\n') line[--n] = '\0';
  b->line = strdup(line);
  for (p = line; nf < 11; nf++) {
    f[nf] = p;
    p = strchr(p, '\t');
    if (p == NULL) { nf++; break; }
    *p++ = '\0';
  }
  if (nf < 11) { free(line); return -1; }
  memset(&b->core, 0, sizeof(b->core));
  b->core.l_qname = strlen(f[0]) + 1;
  put(&d, f[0], strlen(f[0]) + 1);
  b->core.flag = strtol(f[1], NULL, 0);
  b->core.tid = -1;
  for (k = 0; k < fp->header->n_targets; k++) {
    if (0 == strcmp(fp->header->target_name[k], f[2])) { b->core.tid = k; break; }
  }
  b->core.pos = atoi(f[3]) - 1;
  b->core.qual = atoi(f[4]);
  b->core.mtid = -1; b->core.mpos = -1;
  if (0 != strcmp(f[5], "*")) {
    const char *ops = "MIDNSHP=X", *q = f[5]; int nc = 0;
    while (*q) {
      char *e; uint32_t len = strtoul(q, &e, 10), c;
      const char *o = *e ? strchr(ops, *e) : NULL;
      if (o == NULL) break;
      c = len << BAM_CIGAR_SHIFT | (uint32_t)(o - ops);
      put(&d, &c, 4); nc++; q = e + 1;
    }
    b->core.n_cigar = nc;
  }
  while (p != NULL) {          /* the optional fields */
    char *e = strchr(p, '\t');
    if (e) *e++ = '\0';
    put_aux(&d, p);
    p = e;
  }
  b->data = d.s; b->data_len = d.l;
  free(line);
  return (int)n + 1;
}

/* ---- binary mode ---- */

static int gz_all(samfile_t *fp, void *p, unsigned n) { return n == 0 || gzread((gzFile)fp->gz, p, n) == (int)n; }

static int bam_header_read(samfile_t *fp)
{
  bam_header_t *h = fp->header;
  char magic[4]; int32_t l_text, n_ref, i;
  if (!gz_all(fp, magic, 4) || 0 != memcmp(magic, "BAM\1", 4)) return -1;
  if (!gz_all(fp, &l_text, 4) || l_text < 0) return -1;
  h->text = (char*)calloc(1, (size_t)l_text + 1); h->l_text = l_text;
  if (!gz_all(fp, h->text, l_text)) return -1;
  if (!gz_all(fp, &n_ref, 4) || n_ref < 0) return -1;
  for (i = 0; i < n_ref; i++) {
    int32_t l_name, l_ref; char *name;
    if (!gz_all(fp, &l_name, 4) || l_name < 1) return -1;
    name = (char*)calloc(1, (size_t)l_name + 1);
    if (!gz_all(fp, name, l_name) || !gz_all(fp, &l_ref, 4)) { free(name); return -1; }
    header_add_target(h, name, strlen(name));
    free(name);
  }
  return 0;
}

static int bam_read(samfile_t *fp, bam1_t *b)
{
  int32_t block_size; uint32_t x[8];
  if (!gz_all(fp, &block_size, 4) || block_size < 32) return -1;
  if (!gz_all(fp, x, 32)) return -1;
  b->core.tid = (int32_t)x[0]; b->core.pos = (int32_t)x[1];
  b->core.bin = x[2] >> 16; b->core.qual = x[2] >> 8 & 0xff; b->core.l_qname = x[2] & 0xff;
  b->core.flag = x[3] >> 16; b->core.n_cigar = x[3] & 0xffff;
  b->core.l_qseq = (int32_t)x[4]; b->core.mtid = (int32_t)x[5]; b->core.mpos = (int32_t)x[6]; b->core.isize = (int32_t)x[7];
  b->data_len = block_size - 32;
  b->data = (uint8_t*)malloc(b->data_len + 1);
  if (!gz_all(fp, b->data, b->data_len)) return -1;
  return block_size + 4;
}

/* ---- what dwgsim_eval.c calls ---- */

samfile_t *samopen(const char *fn, const char *mode, const void *aux)
{
  samfile_t *fp = (samfile_t*)calloc(1, sizeof(samfile_t));
  int is_stdio = (0 == strcmp(fn, "-"));
  if (mode[0] == 'w') {          /* "wh": SAM text with the header, to stdout */
    fp->mode = 'w'; fp->fp = stdout; fp->header = (bam_header_t*)aux;
    if (strchr(mode, 'h') && fp->header && fp->header->text) fwrite(fp->header->text, 1, fp->header->l_text, stdout);
    return fp;
  }
  fp->header = (bam_header_t*)calloc(1, sizeof(bam_header_t)); fp->own_header = 1;
  if (strchr(mode, 'b')) {
    fp->mode = 'b';
    fp->gz = is_stdio ? gzdopen(fileno(stdin), "rb") : gzopen(fn, "rb");
    if (fp->gz == NULL || bam_header_read(fp) < 0) { samclose(fp); return NULL; }
  } else {
    fp->mode = 'r';
    fp->fp = is_stdio ? stdin : fopen(fn, "r");
    if (fp->fp == NULL) { samclose(fp); return NULL; }
    text_header_read(fp);
  }
  return fp;
}

int samread(samfile_t *fp, bam1_t *b)
{
  return fp->mode == 'b' ? bam_read(fp, b) : text_read(fp, b);
}

int samwrite(samfile_t *fp, const bam1_t *b)
{
  return b->line ? fprintf(fp->fp, "%s\n", b->line) : fprintf(fp->fp, "(a BAM record: its text is not restated)\n");
}

void samclose(samfile_t *fp)
{
  if (fp == NULL) return;
  if (fp->mode == 'w') fflush(fp->fp);
  else if (fp->mode == 'r' && fp->fp && fp->fp != stdin) fclose(fp->fp);
  if (fp->gz) gzclose((gzFile)fp->gz);
  if (fp->own_header) header_destroy(fp->header);
  free(fp);
}

/* the size of the aux value at s (s[0] is its type), or -1 when it cannot be walked within end */
static long aux_size(const uint8_t *s, const uint8_t *end)
{
  switch (s[0]) {
    case 'A': case 'c': case 'C': return 2;
    case 's': case 'S': return 3;
    case 'i': case 'I': case 'f': return 5;
    case 'Z': case 'H': { const uint8_t *z = (const uint8_t*)memchr(s + 1, 0, end - (s + 1)); return z ? z + 1 - s : -1; }
    case 'B': {
      uint32_t cnt;
      if (end - s < 6 || !b_size(s[1])) return -1;
      memcpy(&cnt, s + 2, 4);
      return 6 + (long)b_size(s[1]) * cnt;
    }
  }
  return -1;
}

uint8_t *bam_aux_get(const bam1_t *b, const char tag[2])
{
  const uint8_t *s = bam1_aux(b), *end = b->data + b->data_len;
  while (end - s >= 3) {
    long n = aux_size(s + 2, end);
    if (n < 0 || n > end - (s + 2)) break;
    if (s[0] == (uint8_t)tag[0] && s[1] == (uint8_t)tag[1]) return (uint8_t*)s + 2;
    s += 2 + n;
  }
  return NULL;
}

int32_t bam_aux2i(const uint8_t *s)
{
  int8_t c; int16_t h; uint16_t H; int32_t i; uint32_t I;
  switch (s[0]) {
    case 'c': memcpy(&c, s + 1, 1); return c;
    case 'C': return s[1];
    case 's': memcpy(&h, s + 1, 2); return h;
    case 'S': memcpy(&H, s + 1, 2); return H;
    case 'i': memcpy(&i, s + 1, 4); return i;
    case 'I': memcpy(&I, s + 1, 4); return (int32_t)I;
  }
  return 0;
}
