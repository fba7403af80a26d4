/* gac_netfile.c -- .net text: kent net reader tree and NetFilterNonNested
 * (see gac_netfile.h for the reference semantics restated here). */
#define _GNU_SOURCE
#include "gac_netfile.h"

#include <ctype.h>
#include <limits.h>
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <stdatomic.h>
#include <string.h>

#include "gac_tool.h"
#include "host/gac_host.h"

/* ------------------------------------------------------------ lines */
void gt_lines_push(gt_lines *l, char *s) {
    if (l->n == l->cap) {
        l->cap = l->cap ? l->cap * 2 : 1024;
        l->line = realloc(l->line, (size_t)l->cap * sizeof(char *));
    }
    l->line[l->n++] = s;
}

void gt_lines_read(const char *path, gt_lines *l) {
    memset(l, 0, sizeof(*l));
    FILE *f = gt_must_open(path, "r");
    size_t cap = 1 << 20, len = 0;
    char *buf = malloc(cap + 1);
    size_t r;
    while ((r = fread(buf + len, 1, cap - len, f)) > 0) {
        len += r;
        if (len == cap) {
            cap *= 2;
            buf = realloc(buf, cap + 1);
        }
    }
    if (f != stdin)
        fclose(f);
    buf[len] = 0;
    l->buf = buf;
    char *p = buf, *end = buf + len;
    while (p < end) {
        char *nl = memchr(p, '\n', end - p);
        if (nl)
            *nl = 0;
        if (l->n == l->cap) {
            l->cap = l->cap ? l->cap * 2 : 1024;
            l->line = realloc(l->line, (size_t)l->cap * sizeof(char *));
        }
        l->line[l->n++] = p;
        p = nl ? nl + 1 : end;
    }
}

void gt_lines_free(gt_lines *l) {
    if (!l->buf)
        for (int64_t i = 0; i < l->n; ++i)
            free(l->line[i]);
    free(l->line);
    free(l->buf);
    memset(l, 0, sizeof(*l));
}

/* ------------------------------------------------------------ net tree */
/* Every line is classified and parsed as a fill/gap line on all threads
 * first (pre_line); the tree is then built by the reference's recursion in
 * one serial pass that only reads those records.  A line the fast parse
 * cannot settle (or an error) goes through fill_from_line as before, which
 * aborts with the reference's message at the same point of the serial
 * pass. */
typedef struct pre_line {
    int32_t lead;    /* leading spaces */
    uint8_t real;    /* lineFileNextReal keeps it */
    uint8_t ok;      /* fill record parsed (else: fill_from_line decides) */
    gt_fill f;
} pre_line;

typedef struct reader {
    const gt_lines *l;
    int64_t pos;
    const char *what;
    gt_netset *ns;
    const pre_line *pre; /* NULL: parse lines as they come */
} reader;

/* lineFileNextReal: skip blank lines and lines whose first non-blank is '#' */
static char *next_real(reader *r) {
    while (r->pos < r->l->n) {
        if (r->pre) {
            const int64_t i = r->pos++;
            if (r->pre[i].real)
                return r->l->line[i];
            continue;
        }
        char *s = r->l->line[r->pos++];
        const char *p = s;
        while (isspace((unsigned char)*p))
            ++p;
        if (*p != 0 && *p != '#')
            return s;
    }
    return NULL;
}

static int32_t need_num(reader *r, char **w, int i) {
    char *end;
    long v = strtol(w[i], &end, 10);
    if (*w[i] == 0 || *end != 0)
        gt_abort("Expecting number field %d line %lld of %s, got %s", i + 1, (long long)r->pos,
                 r->what, w[i]);
    return (int32_t)v;
}

/* cnFillFromLine (chainNet.c:86-150): the fields chainCleaner uses */
static int32_t fill_from_line(reader *r, char *line) {
    if (r->pre && r->pre[r->pos - 1].ok) { /* (parsed on the threads) */
        gt_netset *ns = r->ns;
        if (ns->nf == ns->fcap) {
            ns->fcap = ns->fcap ? ns->fcap * 2 : 4096;
            ns->fills = realloc(ns->fills, (size_t)ns->fcap * sizeof(gt_fill));
        }
        ns->fills[ns->nf] = r->pre[r->pos - 1].f;
        return (int32_t)ns->nf++;
    }
    char *w[64];
    char *copy = strdup(line);
    int wc = gac_chop_white(copy, w, 64);
    if (wc < 7)
        gt_abort("Expecting 7 words line %lld of %s got %d", (long long)r->pos, r->what, wc);
    gt_netset *ns = r->ns;
    if (ns->nf == ns->fcap) {
        ns->fcap = ns->fcap ? ns->fcap * 2 : 4096;
        ns->fills = realloc(ns->fills, (size_t)ns->fcap * sizeof(gt_fill));
    }
    gt_fill *f = &ns->fills[ns->nf];
    memset(f, 0, sizeof(*f));
    f->child = f->next = -1;
    f->tstart = need_num(r, w, 1);
    f->tsize = need_num(r, w, 2);
    need_num(r, w, 5);
    need_num(r, w, 6);
    for (int i = 7; i < wc; i += 2) {
        if (i + 1 >= wc)
            break;
        if (strcmp(w[i], "score") == 0)
            f->score = atof(w[i + 1]);
        else if (strcmp(w[i], "type") == 0)
            ;
        else {
            int32_t v = need_num(r, w, i + 1);
            if (strcmp(w[i], "id") == 0)
                f->chain_id = v;
        }
    }
    free(copy);
    return (int32_t)ns->nf++;
}

static int lead_spaces(const char *s) {
    int d = 0;
    while (s[d] == ' ')
        ++d;
    return d;
}

/* need_num's test on a token: the whole token is a decimal long (strtol) */
static int tok_num(const char *t, int len, int32_t *v) {
    char b[64];
    if (len <= 0 || len >= (int)sizeof(b))
        return 0;
    memcpy(b, t, (size_t)len);
    b[len] = 0;
    char *end;
    const long x = strtol(b, &end, 10);
    if (*end != 0)
        return 0;
    *v = (int32_t)x;
    return 1;
}

/* fill_from_line's fields without the copy: 1 = parsed exactly as it
 * would; 0 = let fill_from_line handle it (errors, odd tokens) */
static int fast_fill(const char *line, gt_fill *f) {
    const char *w[64];
    int wl[64], wc = 0;
    const char *p = line;
    while (wc < 64) { /* gac_chop_white */
        while (*p && isspace((unsigned char)*p))
            ++p;
        if (*p == 0)
            break;
        w[wc] = p;
        while (*p && !isspace((unsigned char)*p))
            ++p;
        wl[wc] = (int)(p - w[wc]);
        ++wc;
    }
    if (wc < 7)
        return 0;
    memset(f, 0, sizeof(*f));
    f->child = f->next = -1;
    int32_t v;
    if (!tok_num(w[1], wl[1], &f->tstart) || !tok_num(w[2], wl[2], &f->tsize) ||
        !tok_num(w[5], wl[5], &v) || !tok_num(w[6], wl[6], &v))
        return 0;
    for (int i = 7; i < wc; i += 2) {
        if (i + 1 >= wc)
            break;
        if (wl[i] == 5 && memcmp(w[i], "score", 5) == 0) {
            char b[64];
            if (wl[i + 1] >= (int)sizeof(b))
                return 0;
            memcpy(b, w[i + 1], (size_t)wl[i + 1]);
            b[wl[i + 1]] = 0;
            f->score = atof(b);
        } else if (wl[i] == 4 && memcmp(w[i], "type", 4) == 0) {
        } else {
            if (!tok_num(w[i + 1], wl[i + 1], &v))
                return 0;
            if (wl[i] == 2 && memcmp(w[i], "id", 2) == 0)
                f->chain_id = v;
        }
    }
    return 1;
}

typedef struct pre_job {
    const gt_lines *l;
    pre_line *pre;
    int64_t per;
    _Atomic int64_t next;
} pre_job;

static void *pre_thread(void *arg) {
    pre_job *J = arg;
    for (;;) {
        const int64_t a = atomic_fetch_add(&J->next, 1) * J->per;
        if (a >= J->l->n)
            return NULL;
        const int64_t b = a + J->per < J->l->n ? a + J->per : J->l->n;
        for (int64_t i = a; i < b; ++i) {
            const char *s = J->l->line[i];
            pre_line *x = &J->pre[i];
            const char *q = s;
            while (isspace((unsigned char)*q))
                ++q;
            x->real = *q != 0 && *q != '#';
            x->lead = lead_spaces(s);
            x->ok = x->real && x->lead > 0 && fast_fill(s, &x->f);
        }
    }
}

/* cnFillRead (chainNet.c:152-178) */
static int32_t read_list(reader *r) {
    int depth = 0;
    int32_t head = -1, tail = -1, fill = -1;
    for (;;) {
        char *line = next_real(r);
        if (!line)
            break;
        const int d = r->pre ? r->pre[r->pos - 1].lead : lead_spaces(line);
        if (fill < 0)
            depth = d;
        if (d < depth) {
            --r->pos; /* lineFileReuse */
            break;
        }
        if (d > depth) {
            --r->pos;
            const int32_t c = read_list(r);
            r->ns->fills[fill].child = c;
        } else {
            fill = fill_from_line(r, line);
            if (tail < 0)
                head = fill;
            else
                r->ns->fills[tail].next = fill;
            tail = fill;
        }
    }
    return head;
}

void gt_net_parse(const gt_lines *l, const char *what, gt_netset *ns) {
    memset(ns, 0, sizeof(*ns));
    reader r = {l, 0, what, ns, NULL};
    pre_line *pre = NULL;
    if (l->n >= 65536 && !getenv("GAC_NET_PARSE_SERIAL")) {
        pre = malloc((size_t)l->n * sizeof(pre_line));
        pre_job J = {l, pre, 8192, 0};
        atomic_init(&J.next, 0);
        gac_run_threads(gt_threads(), pre_thread, &J);
        r.pre = pre;
    }
    char *line;
    while ((line = next_real(&r)) != NULL) {
        if (strncmp(line, "net ", 4) != 0)
            gt_abort("Expecting 'net' first word of line %lld of %s", (long long)r.pos, what);
        char *w[3];
        char *copy = strdup(line);
        int wc = gac_chop_white(copy, w, 3);
        if (wc < 3)
            gt_abort("Expecting 3 words line %lld of %s got %d", (long long)r.pos, what, wc);
        if (ns->n == ns->cap) {
            ns->cap = ns->cap ? ns->cap * 2 : 64;
            ns->nets = realloc(ns->nets, (size_t)ns->cap * sizeof(gt_net1));
        }
        gt_net1 *n = &ns->nets[ns->n++];
        n->name = strdup(w[1]);
        n->size = need_num(&r, w, 2);
        free(copy);
        n->first = read_list(&r);
    }
    free(pre);
}

void gt_netset_free(gt_netset *ns) {
    for (int32_t i = 0; i < ns->n; ++i)
        free(ns->nets[i].name);
    free(ns->nets);
    free(ns->fills);
    memset(ns, 0, sizeof(*ns));
}

/* ------------------------------------------------------------ full-field nets */
/* cnFillFromLine (chainNet.c:86-150) of one line, without touching it and
 * without aborting: NF_OK, or what the reference (or this tool) complains
 * about first, in its order of checks */
enum { NF_OK = 0, NF_WORDS, NF_NUM, NF_NOVAL };
typedef struct nf_err {
    int kind, field, wc; /* field: 1-based word (NF_NUM), the name's word (NF_NOVAL) */
    const char *tok;
    int tok_len;
} nf_err;

/* lineFileNeedNum (linefile.c:1015-1025): a '-' or a digit first, then atoi */
static int ref_num(const char *t, int32_t *v) {
    if (*t != '-' && !isdigit((unsigned char)*t))
        return 0;
    *v = (int32_t)strtol(t, NULL, 10); /* (the token ends at white space or NUL) */
    return 1;
}

static int tok_is(const char *t, int len, const char *name) {
    return (int)strlen(name) == len && memcmp(t, name, (size_t)len) == 0;
}

static int nfill_parse(const char *line, gt_nfill *f, nf_err *e) {
    const char *w[64];
    int wl[64], wc = 0;
    const char *p = line;
    while (wc < 64) { /* chopLine: at most 64 words */
        while (*p && isspace((unsigned char)*p))
            ++p;
        if (*p == 0)
            break;
        w[wc] = p;
        while (*p && !isspace((unsigned char)*p))
            ++p;
        wl[wc] = (int)(p - w[wc]);
        ++wc;
    }
    e->wc = wc;
    if (wc < 7)
        return e->kind = NF_WORDS;
    f->score = 0;
    f->chain_id = f->ali = 0;
    f->qover = f->qfar = f->qdup = f->type = -1;
    f->tn = f->qn = f->tr = f->qr = f->tnewr = f->qnewr = f->toldr = f->qoldr = f->ttrf = f->qtrf = -1;
    f->child = f->next = f->parent = -1;
    f->level = 0;
    f->qname = -1;
    f->type_off = f->type_len = 0;
#define NF_NEED(ix, dst)                 \
    if (!ref_num(w[ix], dst)) {          \
        e->field = (ix) + 1;             \
        e->tok = w[ix];                  \
        e->tok_len = wl[ix];             \
        return e->kind = NF_NUM;         \
    }
    NF_NEED(1, &f->tstart)
    NF_NEED(2, &f->tsize)
    f->q_off = (int32_t)(w[3] - line);
    f->q_len = wl[3];
    f->qstrand = w[4][0];
    NF_NEED(5, &f->qstart)
    NF_NEED(6, &f->qsize)
    static const struct {
        const char *name;
        size_t off;
    } k_int[] = {
        {"id", offsetof(gt_nfill, chain_id)}, {"ali", offsetof(gt_nfill, ali)},
        {"tN", offsetof(gt_nfill, tn)},       {"qN", offsetof(gt_nfill, qn)},
        {"tR", offsetof(gt_nfill, tr)},       {"qR", offsetof(gt_nfill, qr)},
        {"tNewR", offsetof(gt_nfill, tnewr)}, {"qNewR", offsetof(gt_nfill, qnewr)},
        {"tOldR", offsetof(gt_nfill, toldr)}, {"qOldR", offsetof(gt_nfill, qoldr)},
        {"tTrf", offsetof(gt_nfill, ttrf)},   {"qTrf", offsetof(gt_nfill, qtrf)},
        {"qOver", offsetof(gt_nfill, qover)}, {"qFar", offsetof(gt_nfill, qfar)},
        {"qDup", offsetof(gt_nfill, qdup)},
    };
    for (int i = 7; i < wc; i += 2) {
        if (i + 1 >= wc) { /* the reference reads words[i + 1] all the same */
            e->field = i + 1;
            e->tok = w[i];
            e->tok_len = wl[i];
            return e->kind = NF_NOVAL;
        }
        if (tok_is(w[i], wl[i], "score"))
            f->score = atof(w[i + 1]);
        else if (tok_is(w[i], wl[i], "type")) {
            f->type_off = (int32_t)(w[i + 1] - line);
            f->type_len = wl[i + 1];
        } else {
            int32_t v;
            NF_NEED(i + 1, &v)
            for (size_t k = 0; k < sizeof(k_int) / sizeof(k_int[0]); ++k)
                if (tok_is(w[i], wl[i], k_int[k].name)) {
                    *(int32_t *)((char *)f + k_int[k].off) = v;
                    break;
                }
        }
    }
#undef NF_NEED
    return e->kind = NF_OK;
}

static void nfill_abort(const nf_err *e, int64_t line_no, const char *what) {
    if (e->kind == NF_WORDS)
        gt_abort("Expecting at least 7 words line %lld of %s got %d", (long long)line_no, what, e->wc);
    if (e->kind == NF_NUM)
        gt_abort("Expecting number field %d line %lld of %s, got %.*s", e->field,
                 (long long)line_no, what, e->tok_len, e->tok);
    gt_abort("Field %.*s without a value line %lld of %s", e->tok_len, e->tok, (long long)line_no,
             what);
}

typedef struct npre_job {
    const gt_lines *l;
    gt_nfill *f;
    int64_t per;
    _Atomic int64_t next;
} npre_job;

static void *npre_thread(void *arg) {
    npre_job *J = arg;
    for (;;) {
        const int64_t a = atomic_fetch_add(&J->next, 1) * J->per;
        if (a >= J->l->n)
            return NULL;
        const int64_t b = a + J->per < J->l->n ? a + J->per : J->l->n;
        for (int64_t i = a; i < b; ++i) {
            const char *s = J->l->line[i];
            gt_nfill *x = &J->f[i];
            const char *q = s;
            while (isspace((unsigned char)*q)) /* lineFileNextReal */
                ++q;
            x->real = *q != 0 && *q != '#';
            x->lead = lead_spaces(s);
            nf_err e;
            x->ok = x->real && x->lead > 0 && nfill_parse(s, x, &e) == NF_OK;
        }
    }
}

typedef struct nreader {
    const gt_lines *l;
    int64_t pos; /* lines consumed: the 1-based number of the last one read */
    const char *what;
    gt_nnetset *ns;
} nreader;

static int64_t nnext_real(nreader *r) { /* the line's index or -1 */
    while (r->pos < r->l->n)
        if (r->ns->fills[r->pos++].real)
            return r->pos - 1;
    return -1;
}

/* cnFillRead (chainNet.c:152-185): a deeper line opens the child list of the
 * last record of this list -- replacing a list that record already had, when a
 * line comes back to a level between the two */
static int32_t nread_list(nreader *r) {
    gt_nnetset *ns = r->ns;
    int depth = 0;
    int32_t head = -1, tail = -1, fill = -1;
    for (;;) {
        const int64_t i = nnext_real(r);
        if (i < 0)
            break;
        gt_nfill *f = &ns->fills[i];
        const int d = f->lead;
        if (fill < 0)
            depth = d;
        if (d < depth) {
            --r->pos; /* lineFileReuse */
            break;
        }
        if (d > depth) {
            --r->pos;
            const int32_t c = nread_list(r);
            ns->fills[fill].child = c;
            continue;
        }
        if (!f->ok) { /* a line at level 0, or one the reference refuses */
            nf_err e;
            if (nfill_parse(r->l->line[i], f, &e) != NF_OK)
                nfill_abort(&e, i + 1, r->what);
        }
        const char *s = r->l->line[i];
        f->qname = gt_names_add(ns->qnames, s + f->q_off, (size_t)f->q_len);
        if (f->type_len)
            f->type = gt_names_add(ns->types, s + f->type_off, (size_t)f->type_len);
        fill = (int32_t)i;
        if (tail < 0)
            head = fill;
        else
            ns->fills[tail].next = fill;
        tail = fill;
    }
    return head;
}

/* pre-order over a sibling list: level, parent, the output order */
static void norder(gt_nnetset *ns, int32_t f, int32_t parent, int32_t level) {
    for (; f >= 0; f = ns->fills[f].next) {
        ns->fills[f].parent = parent;
        ns->fills[f].level = level;
        ns->order[ns->n_order++] = f;
        if (ns->fills[f].child >= 0)
            norder(ns, ns->fills[f].child, f, level + 1);
    }
}

void gt_nnet_parse(const gt_lines *l, const char *what, gt_nnetset *ns) {
    memset(ns, 0, sizeof(*ns));
    if (l->n > INT32_MAX)
        gt_abort("%s: more than %d lines", what, INT32_MAX);
    ns->nl = l->n;
    ns->fills = malloc((size_t)(l->n ? l->n : 1) * sizeof(gt_nfill));
    ns->order = malloc((size_t)(l->n ? l->n : 1) * sizeof(int32_t));
    ns->qnames = calloc(1, sizeof(gt_names));
    ns->types = calloc(1, sizeof(gt_names));
    if (!ns->fills || !ns->order || !ns->qnames || !ns->types)
        gt_abort("Out of memory");
    npre_job J = {l, ns->fills, 8192, 0};
    atomic_init(&J.next, 0);
    const int64_t slices = l->n / J.per + 1;
    gac_run_threads(slices < gt_threads() ? (int)slices : gt_threads(), npre_thread, &J);
    nreader r = {l, 0, what, ns};
    int64_t i;
    while ((i = nnext_real(&r)) >= 0) { /* chainNetRead (chainNet.c:244-264) */
        const char *line = l->line[i];
        if (strncmp(line, "net ", 4) != 0)
            gt_abort("Expecting 'net' first word of line %lld of %s", (long long)r.pos, what);
        char *w[3];
        char *copy = strdup(line);
        const int wc = gac_chop_white(copy, w, 3);
        if (wc < 3)
            gt_abort("Expecting at least 3 words line %lld of %s got %d", (long long)r.pos, what, wc);
        if (ns->n == ns->cap) {
            ns->cap = ns->cap ? ns->cap * 2 : 64;
            ns->nets = realloc(ns->nets, (size_t)ns->cap * sizeof(gt_net1));
        }
        gt_net1 *n = &ns->nets[ns->n++];
        n->name = strdup(w[1]);
        if (!ref_num(w[2], &n->size))
            gt_abort("Expecting number field 3 line %lld of %s, got %s", (long long)r.pos, what, w[2]);
        free(copy);
        n->first = nread_list(&r);
    }
    ns->net_off = malloc((size_t)(ns->n + 1) * sizeof(int64_t));
    for (int32_t k = 0; k < ns->n; ++k) {
        ns->net_off[k] = ns->n_order;
        norder(ns, ns->nets[k].first, -1, 1);
    }
    ns->net_off[ns->n] = ns->n_order;
}

void gt_nnetset_free(gt_nnetset *ns) {
    for (int32_t i = 0; i < ns->n; ++i)
        free(ns->nets[i].name);
    free(ns->nets);
    free(ns->fills);
    free(ns->order);
    free(ns->net_off);
    if (ns->qnames)
        gt_names_free(ns->qnames);
    if (ns->types)
        gt_names_free(ns->types);
    free(ns->qnames);
    free(ns->types);
    memset(ns, 0, sizeof(*ns));
}

/* ---- the typed-net writer */
typedef struct nwrite_job {
    const gt_nnetset *ns;
    const int32_t *qdup;
    const int32_t *item;   /* >= 0: position in order; < 0: ~net */
    const size_t *qlen;    /* by query name id */
} nwrite_job;

static char *put_field(char *p, const char *name, size_t nl, int32_t v) {
    return gt_put_int(gt_put_str(p, name, nl), v);
}

static void nwrite_item(FILE *out, int64_t i, void *arg) {
    const nwrite_job *J = arg;
    const gt_nnetset *ns = J->ns;
    const int32_t it = J->item[i];
    if (it < 0) { /* chainNetWrite (chainNet.c:237-242) */
        fprintf(out, "net %s %d\n", ns->nets[~it].name, ns->nets[~it].size);
        return;
    }
    const gt_nfill *f = &ns->fills[ns->order[it]];
    int32_t qover = f->qover, qfar = f->qfar, qdup = f->qdup;
    const char *type = f->type >= 0 ? ns->types->names[f->type] : NULL;
    if (f->chain_id) { /* rNetSyn (netSyntenic.c:235-267) */
        qdup = J->qdup[it];
        const gt_nfill *par = f->parent >= 0 ? &ns->fills[f->parent] : NULL;
        if (!par)
            type = "top";
        else if (par->qname != f->qname)
            type = "nonSyn";
        else {
            const int64_t fs = f->qstart, fe = fs + f->qsize, ps = par->qstart, pe = ps + par->qsize;
            const int64_t x = (fe < pe ? fe : pe) - (fs > ps ? fs : ps); /* rangeIntersection */
            qover = x > 0 ? (int32_t)x : 0;
            qfar = x > 0 ? 0 : (int32_t)-x;
            type = par->qstrand == f->qstrand ? "syn" : "inv";
        }
    }
    /* cnFillWrite (chainNet.c:187-235), one level of indentation per nesting level */
    const char *qn = ns->qnames->names[f->qname];
    const size_t tl = type ? strlen(type) : 0, need = (size_t)f->level + J->qlen[f->qname] + tl + 1024;
    char small[2048], *buf = need <= sizeof(small) ? small : malloc(need), *p = buf;
    memset(p, ' ', (size_t)f->level);
    p += f->level;
    p = f->chain_id ? gt_put_str(p, "fill", 4) : gt_put_str(p, "gap", 3);
    p = gt_put_int(p, f->tstart);
    p = gt_put_int(p, f->tsize);
    p = gt_put_str(p, qn, J->qlen[f->qname]);
    *p++ = f->qstrand;
    *p++ = ' ';
    p = gt_put_int(p, f->qstart);
    p = gt_put_int(p, f->qsize);
    if (f->chain_id)
        p = put_field(p, "id", 2, f->chain_id);
    if (f->score > 0) {
        p = gt_put_str(p, "score", 5);
        if (f->score < 9007199254740992.0 && f->score == (double)(int64_t)f->score)
            p = gt_put_int(p, (int64_t)f->score);
        else /* (at most 309 digits) */
            p += snprintf(p, 400, "%1.0f ", f->score);
    }
    if (f->ali > 0)
        p = put_field(p, "ali", 3, f->ali);
    if (qover >= 0)
        p = put_field(p, "qOver", 5, qover);
    if (qfar >= 0)
        p = put_field(p, "qFar", 4, qfar);
    if (qdup >= 0)
        p = put_field(p, "qDup", 4, qdup);
    if (type)
        p = gt_put_str(gt_put_str(p, "type", 4), type, tl);
    static const struct {
        const char *name;
        size_t nl, off;
    } k_tail[] = {
        {"tN", 2, offsetof(gt_nfill, tn)},       {"qN", 2, offsetof(gt_nfill, qn)},
        {"tR", 2, offsetof(gt_nfill, tr)},       {"qR", 2, offsetof(gt_nfill, qr)},
        {"tNewR", 5, offsetof(gt_nfill, tnewr)}, {"qNewR", 5, offsetof(gt_nfill, qnewr)},
        {"tOldR", 5, offsetof(gt_nfill, toldr)}, {"qOldR", 5, offsetof(gt_nfill, qoldr)},
        {"tTrf", 4, offsetof(gt_nfill, ttrf)},   {"qTrf", 4, offsetof(gt_nfill, qtrf)},
    };
    for (size_t k = 0; k < sizeof(k_tail) / sizeof(k_tail[0]); ++k) {
        const int32_t v = *(const int32_t *)((const char *)f + k_tail[k].off);
        if (v >= 0)
            p = put_field(p, k_tail[k].name, k_tail[k].nl, v);
    }
    p[-1] = '\n'; /* every piece above ends in one space */
    fwrite(buf, 1, (size_t)(p - buf), out);
    if (buf != small)
        free(buf);
}

void gt_nnet_write_typed(FILE *out, const gt_nnetset *ns, const int32_t *qdup) {
    const int64_t n = ns->n + ns->n_order;
    int32_t *item = malloc((size_t)(n ? n : 1) * sizeof(int32_t));
    size_t *qlen = malloc((size_t)(ns->qnames->n ? ns->qnames->n : 1) * sizeof(size_t));
    if (!item || !qlen)
        gt_abort("Out of memory");
    for (int32_t q = 0; q < ns->qnames->n; ++q)
        qlen[q] = strlen(ns->qnames->names[q]);
    int64_t m = 0;
    for (int32_t k = 0; k < ns->n; ++k) {
        item[m++] = ~k;
        for (int64_t o = ns->net_off[k]; o < ns->net_off[k + 1]; ++o)
            item[m++] = (int32_t)o;
    }
    nwrite_job J = {ns, qdup, item, qlen};
    gt_par_write(out, n, nwrite_item, &J);
    free(item);
    free(qlen);
}

/* ------------------------------------------------------------ NetFilterNonNested */
/* the script's fill/gap pattern /^([ ]+)([fill|gap].*)/: spaces, then one of
 * the characters f i l | g a p; returns the space count or -1 */
static int level_of(const char *s) {
    int d = lead_spaces(s);
    if (d == 0 || !strchr("fil|gap", s[d]) || s[d] == 0)
        return -1;
    return d;
}

/* Perl's numeric value of a decimal field (as used by the script's >=) */
static double field_num(const char *s) { return atof(s); }

void gt_netfilter_nonnested(const gt_lines *in, const char *what, double s1, double t1,
                            double q1, double s2, double t2, double q2, gt_lines *out) {
    /* mode "12": an unset set 2 (all zero) -> INT_MAX; an unset set 1 -> INT_MAX */
    if (s2 == 0 && t2 == 0 && q2 == 0)
        s2 = t2 = q2 = INT_MAX;
    if (s1 == 0 && t1 == 0 && q1 == 0)
        s1 = t1 = q1 = INT_MAX;
    const double sc[2] = {s1, s2}, ts[2] = {t1, t2}, qs[2] = {q1, q2};
    gt_netfilter_sets(in, what, 2, sc, ts, qs, out);
}

void gt_netfilter_sets(const gt_lines *in, const char *what, int nsets, const double *set_score,
                       const double *set_t, const double *set_q, gt_lines *out) {
    gt_netfilter_opts o = {nsets, set_score, set_t, set_q, 0, 0, 0, INT_MAX, INT_MAX};
    gt_netfilter(in, what, &o, out);
}

/* first match of /<key>(X+) / in s (X: \w or \d) -- or, with at_end, of
 * /<key>(X+)$/; the value as a string in buf */
static int find_field(const char *s, const char *key, int word, int at_end, char *buf,
                      size_t cap) {
    const size_t kl = strlen(key);
    for (const char *p = strstr(s, key); p; p = strstr(p + 1, key)) {
        const char *v = p + kl, *q = v;
        while (*q && (word ? (isalnum((unsigned char)*q) || *q == '_') : isdigit((unsigned char)*q)))
            ++q;
        if (q == v || (at_end ? *q != 0 : *q != ' '))
            continue;
        snprintf(buf, cap, "%.*s", (int)(q - v), v);
        return 1;
    }
    return 0;
}

/* Level2IsSkipped (a perl hash: absent = 0) */
typedef struct lvmap {
    char *v;
    int n;
} lvmap;

static int lv_get(const lvmap *m, int k) { return k >= 0 && k < m->n ? m->v[k] : 0; }

static void lv_set(lvmap *m, int k, int x) {
    if (k < 0)
        return;
    if (k >= m->n) {
        const int n2 = k + 64;
        m->v = realloc(m->v, (size_t)n2);
        memset(m->v + m->n, 0, (size_t)(n2 - m->n));
        m->n = n2;
    }
    m->v[k] = (char)x;
}

/* testInvSynNet (:330-361) */
static int inv_syn_ok(const gt_netfilter_opts *o, const lvmap *skipped, double score,
                      const char *type, int level) {
    if (lv_get(skipped, level - 2) != 0)
        return 0;
    if (strcmp(type, "inv") == 0)
        return score >= o->keep_inv;
    if (strcmp(type, "syn") == 0)
        return score >= o->keep_syn;
    return 0;
}

/* passesFilter (:365-396) with UCSCsynFilter_nonRecursive (:268-302) and
 * scoreFilter_nonRecursive (:305-327) */
static int passes(const gt_netfilter_opts *o, const lvmap *skipped, double score, double tsz,
                  double qsz, const char *type, double ali, double qfar, int level) {
    if (o->ucsc) {
        if (!*type)
            gt_abort("No type field, please run input net through netSyntenic");
        if (score >= 200000 && tsz >= 20000 && ali >= 10000) /* minSynScore/Size/Ali */
            return 1;
        if (strcmp(type, "top") == 0)
            return score >= 300000; /* minTopScore */
        if (strcmp(type, "nonSyn") == 0)
            return 0;
        if (qfar > 200000) /* maxFar */
            return 0;
        return inv_syn_ok(o, skipped, score, type, level);
    }
    if (o->score_filter) {
        if (!*type)
            gt_abort("No type field, please run input net through netSyntenic");
        if (score >= o->min_score1)
            return 1;
        if (strcmp(type, "top") == 0 || strcmp(type, "nonSyn") == 0)
            return 0;
        return inv_syn_ok(o, skipped, score, type, level);
    }
    if (strcmp(type, "syn") == 0 && score >= o->keep_syn)
        return 1;
    if (strcmp(type, "inv") == 0 && score >= o->keep_inv)
        return 1;
    if (o->nsets == 0)
        gt_abort("ERROR: unknown value for filterMode \n");
    for (int k = 0; k < o->nsets; ++k)
        if (score >= o->set_score[k] && tsz >= o->set_t[k] && qsz >= o->set_q[k])
            return 1;
    return 0;
}

void gt_netfilter(const gt_lines *in, const char *what, const gt_netfilter_opts *o,
                  gt_lines *out) {
    memset(out, 0, sizeof(*out));
    const int64_t n = in->n;
    char *skip = calloc(n ? n : 1, 1);
    int *minus = calloc(n ? n : 1, sizeof(int));
    const int want_type = o->keep_syn < INT_MAX || o->keep_inv < INT_MAX || o->ucsc;
    lvmap skipped = {NULL, 0};
    int max_level = 1;
    /* the script keys its per-net counter by the net line's text */
    gt_names netkey;
    memset(&netkey, 0, sizeof(netkey));
    int64_t *kept = calloc(n ? n : 1, sizeof(int64_t)); /* per distinct net line */
    int64_t i = 0;
    for (; i < n; ++i) {
        if (in->line[i][0] == '#')
            continue;
        if (strncmp(in->line[i], "net ", 4) != 0)
            gt_abort("ERROR: expect file to start with net, but got this line instead: %s\n",
                     in->line[i]);
        break;
    }
    int64_t cur = 0;
    if (i < n) {
        cur = gt_names_add(&netkey, in->line[i], strlen(in->line[i]));
        kept[cur] = 0;
    }
    for (int64_t k = i + 1; k < n; ++k) {
        const char *line = in->line[k];
        if (strstr(line, " gap "))
            continue;
        if (strncmp(line, "net ", 4) == 0) {
            cur = gt_names_add(&netkey, line, strlen(line));
            kept[cur] = 0;
            continue;
        }
        const int level = level_of(line);
        if (level < 0)
            gt_abort("ERROR: expect fill or gap in %s\n", line);
        if (!strstr(line, " fill "))
            continue;
        const char *rest = line + level;
        const char *sc = strstr(rest, "score ");
        /* /score (\d+) /: digits followed by a space */
        double score = -1;
        while (sc) {
            const char *p = sc + 6;
            const char *q = p;
            while (isdigit((unsigned char)*q))
                ++q;
            if (q > p && *q == ' ') {
                score = atof(p);
                break;
            }
            sc = strstr(sc + 1, "score ");
        }
        if (score < 0)
            gt_abort("ERROR: no score field is given in this fill line: %s\n", rest);
        /* split / / of the rest: f[2] = tSize, f[6] = qSize */
        char *copy = strdup(rest);
        char *f[8] = {0};
        int nf = 0;
        for (char *tok = copy;;) {
            char *sp = strchr(tok, ' ');
            if (nf < 8)
                f[nf] = tok;
            ++nf;
            if (!sp)
                break;
            *sp = 0;
            tok = sp + 1;
        }
        const double tsz = nf > 2 ? field_num(f[2]) : 0, qsz = nf > 6 ? field_num(f[6]) : 0;
        free(copy);
        char type[64] = "", num[64];
        if (want_type && !find_field(rest, "type ", 1, 0, type, sizeof(type)) &&
            !find_field(rest, "type ", 1, 1, type, sizeof(type)))
            gt_abort("ERROR: parameter -keepSynNetsWithScore/-keepInvNetsWithScore-doUCSCSynFilter is given, but I cannot parse the net type from this fill line: %s\n",
                     rest);
        double ali = 0, qfar = 0;
        if (o->ucsc) {
            if (!find_field(rest, "ali ", 0, 0, num, sizeof(num)))
                gt_abort("ERROR: parameter -doUCSCSynFilter is given, but I cannot parse the ali filed from this fill line: %s\n",
                         rest);
            ali = atof(num);
            if (strcmp(type, "inv") == 0 || strcmp(type, "syn") == 0) {
                if (!find_field(rest, "qFar ", 0, 0, num, sizeof(num)))
                    gt_abort("ERROR: parameter -doUCSCSynFilter is given, but I cannot parse the qFar filed from this syn/inv fill line: %s\n",
                             rest);
                qfar = atof(num);
            }
        }
        if (max_level < level)
            max_level = level;
        if (passes(o, &skipped, score, tsz, qsz, type, ali, qfar, level)) {
            kept[cur]++;
            for (int l = level; l <= max_level; ++l) /* resetLevel2IsSkipped */
                lv_set(&skipped, l, 0);
        } else {
            lv_set(&skipped, level, 1);
            skip[k] = 1;
            /* eraseGapsMarkSkip(k + 1, level) */
            for (int64_t j = k + 1; j < n; ++j) {
                const char *lj = in->line[j];
                if (strncmp(lj, "net ", 4) == 0)
                    break;
                const int cl = level_of(lj);
                if (cl < 0)
                    gt_abort("ERROR: expect fill or gap in %s\n", lj);
                if (cl <= level)
                    break;
                if (cl == level + 1)
                    skip[j] = 1;
                else
                    minus[j] += 2;
            }
        }
    }
    (void)what;
    /* output(): net lines if a fill of theirs is kept, then kept fill/gap
     * lines re-indented */
    for (int64_t k = 0; k < n; ++k) {
        const char *line = in->line[k];
        if (strncmp(line, "net ", 4) == 0) {
            const int32_t key = gt_names_find(&netkey, line);
            if (key >= 0 && kept[key] > 0)
                gt_lines_push(out, strdup(line));
        }
        if (!skip[k]) {
            const int level = level_of(line);
            if (level >= 0) {
                const int cl = level - minus[k];
                const char *rest = line + level;
                const size_t rl = strlen(rest);
                char *s = malloc((size_t)(cl > 0 ? cl : 0) + rl + 1);
                int p = 0;
                for (; p < cl; ++p)
                    s[p] = ' ';
                memcpy(s + p, rest, rl + 1);
                gt_lines_push(out, s);
            }
        }
    }
    free(skip);
    free(minus);
    free(kept);
    free(skipped.v);
    gt_names_free(&netkey);
}
