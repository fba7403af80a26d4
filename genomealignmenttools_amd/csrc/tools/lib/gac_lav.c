/* gac_lav.c -- see gac_lav.h */
#include "gac_lav.h"

#include <ctype.h>
#include <stdlib.h>
#include <string.h>

#include "host/gac_host.h"

/* lineFileNext: the next line without its end, NULL at the end of the file */
static char *next_line(gl_reader *r) {
    if (!*r->cur)
        return NULL;
    char *line = r->cur, *nl = strchr(line, '\n');
    if (nl) {
        *nl = 0;
        if (nl > line && nl[-1] == '\r')
            nl[-1] = 0;
        r->cur = nl + 1;
    } else {
        r->cur = line + strlen(line);
    }
    ++r->line;
    return line;
}

static void unexpected_eof(const gl_reader *r) { gt_abort("Unexpected end of file in %s", r->path); }

static void seek_end_of_stanza(gl_reader *r) {
    for (;;) {
        const char *line = next_line(r);
        if (!line)
            unexpected_eof(r);
        if (line[0] == '}')
            return;
    }
}

/* lineFileNeedNum: a leading '-' or digit, then atoi */
static int need_num(const gl_reader *r, char **words, int ix) {
    const char *a = words[ix];
    if (a[0] != '-' && !isdigit((unsigned char)a[0]))
        gt_abort("Expecting number field %d line %d of %s, got %s", ix + 1, r->line, r->path, a);
    return atoi(a);
}

static void expect_words(const gl_reader *r, int expecting, int got) {
    if (expecting != got)
        gt_abort("Expecting %d words line %d of %s got %d", expecting, r->line, r->path, got);
}

/* lineFileRow of three words: the next line that is neither blank nor a '#'
 * line; 0 at the end of the file */
static int next_row3(gl_reader *r, char **words) {
    char *line;
    while ((line = next_line(r)) != NULL) {
        if (line[0] == '#')
            continue;
        const int n = gac_chop_white(line, words, 3);
        if (n == 0)
            continue;
        if (n < 3)
            expect_words(r, 3, n);
        return 1;
    }
    return 0;
}

static void parse_s(gl_reader *r) {
    char *words[3];
    if (!next_row3(r, words))
        unexpected_eof(r);
    r->t_size = need_num(r, words, 2);
    if (!next_row3(r, words))
        unexpected_eof(r);
    r->q_size = need_num(r, words, 2);
    seek_end_of_stanza(r);
}

/* justChrom (lav.c:35-47): "/dir/chr1.nib:1-100" is chr1 */
static char *just_chrom(char *s) {
    char *e = strstr(s, ".nib:");
    if (!e)
        return s;
    *e = 0;
    e = strrchr(s, '/');
    return e ? e + 1 : s;
}

static char *clone(const char *s) {
    char *c = strdup(s);
    if (!c)
        gt_abort("Out of memory");
    return c;
}

static void parse_h(gl_reader *r) {
    free(r->t_name);
    free(r->q_name);
    r->t_name = r->q_name = NULL;
    r->is_rc = 0;
    for (int i = 0;; ++i) {
        char *line = next_line(r);
        if (!line)
            unexpected_eof(r);
        if (line[0] == '#')
            continue; /* (as in the reference's for loop, the line still counts in i) */
        if (line[0] == '}') {
            if (i < 2)
                gt_abort("Short H stanza line %d of %s", r->line, r->path);
            break;
        }
        /* nextWord: the first word cut off, the rest of the line or NULL */
        char *word = line;
        while (*word && isspace((unsigned char)*word))
            ++word;
        if (!*word)
            gt_abort("Short line %d of %s\n\n", r->line, r->path);
        char *rest = word;
        while (*rest && !isspace((unsigned char)*rest))
            ++rest;
        if (*rest)
            *rest++ = 0;
        else
            rest = NULL;
        ++word; /* the opening '"' and an optional '>' */
        if (*word == '>')
            ++word;
        char *e = strchr(word, '"');
        if (e) {
            *e = 0;
            if (rest)
                ++rest;
        }
        if (i == 0)
            r->t_name = clone(just_chrom(word));
        else if (i == 1)
            r->q_name = clone(just_chrom(word));
        if (rest && strstr(rest, "(reverse"))
            r->is_rc = 1;
    }
}

static void strip_char(char *s, char c) {
    char *w = s;
    for (; *s; ++s)
        if (*s != c)
            *w++ = *s;
    *w = 0;
}

static void parse_d(gl_reader *r) {
    char *line = next_line(r);
    if (!line)
        unexpected_eof(r);
    if (strstr(line, "lastz")) {
        char *words[64];
        strip_char(line, '"');
        const int n = gac_chop_white(line, words, 64);
        fprintf(r->out, "##aligner=%s", words[0]);
        for (int i = 3; i < n; ++i)
            fprintf(r->out, " %s ", words[i]);
        fprintf(r->out, "\n");
        char *aligner = clone(words[0]);
        int32_t mat[16], go = 0, ge = 0;
        char *extra = NULL;
        if (gac_scheme_parse(&r->cur, &r->line, r->path, mat, &go, &ge, &extra) != GAC_OK)
            gt_abort("%s", gac_last_error());
        /* axtScoreSchemeDnaWrite (axt.c:836-872) */
        fprintf(r->out, "##matrix=%s 16", aligner);
        for (int i = 0; i < 16; ++i)
            fprintf(r->out, "%c%d", i ? ',' : ' ', mat[i]);
        fprintf(r->out, "\n##gapPenalties=%s O=%d E=%d\n", aligner, go, ge);
        if (extra) {
            strip_char(extra, ' ');
            strip_char(extra, '"');
            fprintf(r->out, "##blastzParms=%s\n", extra);
        }
        free(extra);
        free(aligner);
    }
    seek_end_of_stanza(r);
}

gl_block *gl_remove_frayed(gl_block *b, int64_t *n) {
    if (*n > 0 && b[0].q_start == b[0].q_end) {
        ++b;
        --*n;
    }
    if (*n > 0 && b[*n - 1].q_start == b[*n - 1].q_end)
        --*n;
    return b;
}

static void parse_a(gl_reader *r) {
    char *line, *words[6];
    int got_score = 0;
    r->nb = 0;
    r->score = -666;
    while ((line = next_line(r)) != NULL) {
        if (line[0] == '#')
            continue;
        if (line[0] == '}')
            break;
        const int wc = gac_chop_white(line, words, 6);
        if (wc == 0)
            continue;
        const char type = words[0][0];
        if (type == 's') {
            if (r->psl)
                expect_words(r, 2, wc);
            got_score = 1;
            r->score = need_num(r, words, 1);
            if (r->psl && r->score_file)
                fprintf(r->score_file, "%d\n", r->score);
        } else if (type == 'l') {
            expect_words(r, 6, wc);
            gl_block b;
            b.t_start = need_num(r, words, 1) - 1;
            b.t_end = need_num(r, words, 3);
            b.q_start = need_num(r, words, 2) - 1;
            b.q_end = need_num(r, words, 4);
            if (b.q_end - b.q_start != b.t_end - b.t_start)
                gt_abort("Block size mismatch line %d of %s", r->line, r->path);
            b.pct = need_num(r, words, 5);
            if (r->psl && b.q_end == b.q_start && b.t_end == b.t_start)
                continue; /* lavToPsl ignores zero length records */
            if (r->nb == r->cap) {
                r->cap = r->cap ? 2 * r->cap : 256;
                r->blk_base = realloc(r->blk_base, (size_t)r->cap * sizeof(gl_block));
                if (!r->blk_base)
                    gt_abort("Out of memory");
            }
            r->blk_base[r->nb++] = b;
        }
    }
    if (!got_score && !r->psl)
        gt_abort("'a' stanza missing score line %d of %s", r->line, r->path);
    r->blk = gl_remove_frayed(r->blk_base, &r->nb);
}

void gl_open(gl_reader *r, const char *path, FILE *out, int psl, FILE *score_file) {
    memset(r, 0, sizeof(*r));
    r->path = path;
    r->out = out;
    r->psl = psl;
    r->score_file = score_file;
    size_t len = 0;
    r->buf = r->cur = gt_slurp(path, &len);
    const char *line = next_line(r);
    if (!line)
        gt_abort("%s is empty", path);
    if (strncmp(line, "#:lav", 5) != 0)
        gt_abort("%s is not a lav file\n\n", path);
}

int gl_next(gl_reader *r) {
    const char *line;
    while ((line = next_line(r)) != NULL) {
        if (!strncmp(line, "s {", 3)) {
            parse_s(r);
        } else if (!strncmp(line, "h {", 3)) {
            parse_h(r);
        } else if (!strncmp(line, "d {", 3)) {
            parse_d(r);
        } else if (!strncmp(line, "a {", 3)) {
            parse_a(r);
            return 1;
        }
    }
    return 0;
}

void gl_close(gl_reader *r) {
    free(r->buf);
    free(r->blk_base);
    free(r->t_name);
    free(r->q_name);
    memset(r, 0, sizeof(*r));
}
