// The taxonomy roll-up of `deSAMBA analysis ana_meta | ana_meta_base` (ana_get_tid, ana_meta,
// ana_meta_base_M2, src/analysis.c:1271-1330,1831-1855) as a library object that a run feeds read by read: the CLI's
// --report, dsb_report_add for callers that keep batches on the device, and `deSAMBA analysis` itself
// (desamba_analysis.c feeds it the SAM file's text).  Pure host code, no HIP.
//
// What is kept to the letter, because it is in the output:
//   - SAM fields are split the way strtok does (runs of separators count as one); AS:i:<n> right after QUAL is the score,
//     the read length is the M/I/S/X total of the CIGAR, the taxid is the second '|' field of RNAME; an RNAME starting
//     with '*' is unclassified; '@' lines are skipped only before the first record (skip_sam_head);
//   - one taxid per read (ana_get_tid): the first record's, moved down to the taxid of a later record of the same name with
//     the same score when that one is a descendant; a first record without score (or with a taxid above max_tid) ends the
//     read at once, its other records then count as reads of their own; the read the input ENDS in is counted only in
//     total_read_number;
//   - counts (ana_meta) or bases weighted by MAPQ (ana_meta_base: reads with coverage * length <= 10 left out) are sorted with
//     the C library's qsort and the reference's comparator, which answers "a < b" with 1 and everything else with 0 -- the
//     order of the children in the printout is whatever glibc's merge sort makes of that -- then added up along the parent
//     links of nodes.dmp and printed depth first, nodes below 0.01 % left out; percentages in single precision.
// The report is a state machine over records: the read being read stays open until a record of another name arrives,
// which is where the last-read rule falls out.  A read the device walked (dsb_read_taxon) enters it as one step.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <new>
#include <string>
#include <vector>
#include "dsb_taxonomy.h"

struct Rec { const char *name; char cls; uint32_t tid, len, score; uint8_t mapq; };

// next token of s in the strtok sense: skip separators, return the token start, cut it at the next separator
static char *tok(char **s, const char *sep)
{
	if (!*s) return NULL;
	char *p = *s + strspn(*s, sep);
	if (!*p) { *s = NULL; return NULL; }
	char *e = p + strcspn(p, sep);
	if (*e) { *e = 0; *s = e + 1; } else *s = NULL;
	return p;
}

// one SAM line (with its '\n') as analysis reads it; the line is cut up in place, r->name points into it
static int parse_sam_line(char *line, Rec *r)
{
	char *s = line, *t;
	if (!(t = tok(&s, "\t"))) return -1;
	r->name = t;
	tok(&s, "\t");                                                         // FLAG
	r->len = 0; r->score = 0; r->tid = 0; r->mapq = 0;
	char *rname = tok(&s, "\t");
	if (!rname || rname[0] == '*') { r->cls = 'U'; return 0; }
	r->cls = 'C';
	tok(&s, "\t");                                                         // POS
	t = tok(&s, "\t"); r->mapq = (uint8_t)(t ? strtoul(t, NULL, 10) : 0);
	char *cigar = tok(&s, "\t");
	for (int k = 0; k < 5; k++) tok(&s, "\t");                             // RNEXT PNEXT TLEN SEQ QUAL
	t = tok(&s, ":");
	if (t && ((t[0] == 'A' && t[1] == 'S') || (t[0] == 'N' && t[1] == 'M'))) {
		tok(&s, ":");
		t = tok(&s, "\t"); r->score = (uint32_t)(t ? strtoul(t, NULL, 10) : 0);
		t = tok(&s, ":");
		if (t && t[0] == 'm' && t[1] == 's') { tok(&s, ":"); t = tok(&s, "\t"); r->score = (uint32_t)(t ? strtoul(t, NULL, 10) : 0); }
	}
	char *q = rname; tok(&q, "|");
	t = tok(&q, "|"); r->tid = (uint32_t)(t ? strtoul(t, NULL, 10) : 0);
	uint32_t total = 0, run = 0;
	for (const char *c = cigar ? cigar : ""; *c; c++) {
		if (*c >= '0' && *c <= '9') run = run * 10 + (uint32_t)(*c - '0');
		else { if (*c == 'M' || *c == 'I' || *c == 'S' || *c == 'X') total += run; run = 0; }
	}
	r->len = total;
	return 0;
}

uint32_t dsb_ref_taxid(const char *name)
{
	if (!name[0] || name[0] == '*' || strpbrk(name, "\t\n")) return DSB_TID_NONE;
	std::string n(name);
	char *q = &n[0]; tok(&q, "|");
	const char *t = tok(&q, "|");
	return (uint32_t)(t ? strtoul(t, NULL, 10) : 0);
}

// ---- nodes.dmp ----
static int load(const char *path, bool check, dsb_taxonomy **out)
{
	if (!path || !out) return DSB_EINVAL;
	FILE *f = fopen(path, "r");
	if (!f) return DSB_EIO;
	char *line = NULL; size_t m = 0; uint32_t last = 0;
	while (getline(&line, &m, f) > 0) { char *s = line, *t = tok(&s, "\t|"); if (t) last = (uint32_t)strtoul(t, NULL, 10); }
	const uint32_t max_tid = last + 1000000u;
	dsb_taxonomy *T = (dsb_taxonomy *)calloc(1, sizeof *T);
	if (T) { T->parent = (uint32_t *)malloc(((size_t)max_tid + 1) * 4); T->rank = (char (*)[20])malloc(((size_t)max_tid + 1) * 20); }
	if (!T || !T->parent || !T->rank) { free(line); fclose(f); dsb_taxonomy_close(T); return DSB_ENOMEM; }
	T->max_tid = max_tid;
	for (uint32_t i = 0; i <= max_tid; i++) { T->parent[i] = DSB_TID_NONE; T->rank[i][0] = 0; }
	rewind(f);
	while (getline(&line, &m, f) > 0) {
		char *s = line, *t = tok(&s, "\t|");
		if (!t) continue;
		const uint32_t tid = (uint32_t)strtoul(t, NULL, 10);
		char *p = tok(&s, "\t|"), *r = tok(&s, "\t|");
		if (tid > max_tid || !p) continue;                                  // (the reference writes out of bounds here)
		T->parent[tid] = (uint32_t)strtoul(p, NULL, 10);
		if (r) { strncpy(T->rank[tid], r, sizeof T->rank[tid] - 1); T->rank[tid][sizeof T->rank[tid] - 1] = 0; }
	}
	free(line); fclose(f);
	T->parent[1] = 0; strcpy(T->rank[1], "root"); strcpy(T->rank[0], "CLY_FAIL");
	if (check) {
		// depth[t] = parent links followed from t before a walk stops (at a taxid < 1, DSB_TID_NONE or above max_tid);
		// a chain that comes back to a taxid on it is a cycle
		std::vector<int32_t> depth((size_t)max_tid + 1, -1);
		std::vector<uint32_t> path;
		auto valid = [&](uint32_t p) { return p >= 1 && p != DSB_TID_NONE && p <= max_tid; };
		for (uint32_t t = 1; t <= max_tid; t++) {
			if (depth[t] >= 0) continue;
			path.clear();
			uint32_t p = t;
			while (valid(p) && depth[p] == -1) { depth[p] = -2; path.push_back(p); p = T->parent[p]; }
			if (valid(p) && depth[p] == -2) { dsb_taxonomy_close(T); return DSB_EINVAL; }
			int32_t d = valid(p) ? depth[p] : -1;
			for (size_t k = path.size(); k-- > 0;) { depth[path[k]] = ++d; if ((uint32_t)d > T->max_depth) T->max_depth = (uint32_t)d; }
		}
		T->acyclic = true;
		// the depth is kept for the rooted taxids: a chain that stops at taxid 1 (parent[1] = 0) counted its links to
		// it; a chain that stopped anywhere else is unrooted, and so is every taxid above it.  Parents come before children here
		// only along a chain, so rootedness is settled by a second pass in ascending depth order: a node is rooted when it is 1 or
		// its parent is.
		T->depth = (uint16_t *)malloc(((size_t)max_tid + 1) * 2);
		if (!T->depth) { dsb_taxonomy_close(T); return DSB_ENOMEM; }
		std::vector<std::vector<uint32_t>> by_depth((size_t)T->max_depth + 1);
		for (uint32_t t = 1; t <= max_tid; t++) by_depth[(size_t)depth[t]].push_back(t);
		T->depth[0] = DSB_DEPTH_UNROOTED;
		for (uint32_t d = 0; d <= T->max_depth; d++)
			for (uint32_t t : by_depth[d]) {
				const uint32_t p = T->parent[t];
				const bool rooted = d < DSB_DEPTH_UNROOTED && (t == 1 || (d > 0 && valid(p) && T->depth[p] != DSB_DEPTH_UNROOTED));
				T->depth[t] = rooted ? (uint16_t)d : (uint16_t)DSB_DEPTH_UNROOTED;
			}
	}
	*out = T;
	return DSB_OK;
}
extern "C" int dsb_taxonomy_load(const char *path, dsb_taxonomy **tx) { return load(path, true, tx); }
extern "C" int dsb_taxonomy_load_any(const char *path, dsb_taxonomy **tx) { return load(path, false, tx); }
extern "C" void dsb_taxonomy_close(dsb_taxonomy *T) { if (T) { free(T->parent); free(T->rank); free(T->depth); free(T); } }
extern "C" uint32_t dsb_taxonomy_max_tid(const dsb_taxonomy *T) { return T ? T->max_tid : 0; }
extern "C" uint32_t dsb_taxonomy_parent(const dsb_taxonomy *T, uint32_t tid) { return (T && tid <= T->max_tid) ? T->parent[tid] : DSB_TID_NONE; }

// is `tid` (a record's taxid) at or below `held`?  The walk of ana_get_tid.
static bool descends(const dsb_taxonomy *T, uint32_t tid, uint32_t held)
{
	for (uint32_t p = tid;;) {
		if (p == held) return true;
		if (p < 1 || p == DSB_TID_NONE || p > T->max_tid) return false;
		p = T->parent[p];
	}
}

// ---- the report ----
struct dsb_report {
	const dsb_taxonomy *T;
	std::vector<uint32_t> count; std::vector<uint64_t> base, mq;
	int total_reads = 0; uint64_t total_base = 0, low_n = 0, low_base = 0; float coverage = 0;
	bool any = false, head = true;
	bool open = false; std::string name; uint32_t tid = 0, score = 0; int map_q = 0, read_len = 0;   // the read being read
	std::string line;                                        // scratch: one line of text
	std::vector<char> sam;                                   // scratch: the SAM text of a read walked on the host
};

static void close_read(dsb_report *R)
{
	R->open = false;
	if (R->tid == 0) return;
	R->count[R->tid]++;
	if (R->coverage * R->read_len > 10) {
		R->total_base += (uint64_t)R->read_len; R->base[R->tid] += (uint64_t)R->read_len; R->mq[R->tid] += (uint64_t)(R->read_len * R->map_q);
		if (R->coverage < 0.08) { R->low_base += (uint64_t)R->read_len; R->low_n++; }
	}
}

// a read starts with this record (or device record): total_read_number counts it whether or not it is ever closed
static void start_read(dsb_report *R, const char *name, char cls, uint32_t tid, uint32_t score, uint32_t len, uint8_t mapq)
{
	R->any = true; R->total_reads++;
	R->map_q = mapq; R->read_len = (int)len; R->tid = 0; R->score = 0;
	if (cls != 'C') return;
	R->open = true; R->name = name;
	if (tid <= R->T->max_tid) { R->tid = tid; R->score = score; R->coverage = len > 0 ? (float)score / len : 0; }
}

static void feed_record(dsb_report *R, const Rec &r)
{
	if (R->open) {
		if (R->name != r.name || R->score == 0) close_read(R);
		else {
			if (r.score != R->score || r.tid > R->T->max_tid) return;
			if (descends(R->T, r.tid, R->tid)) R->tid = r.tid;
			return;
		}
	}
	start_read(R, r.name, r.cls, r.tid, r.score, r.len, r.mapq);
}

static void feed_line(dsb_report *R, char *line)
{
	if (R->head && line[0] == '@') return;                   // header lines at the top only
	R->head = false;
	Rec r;
	if (parse_sam_line(line, &r) == 0) feed_record(R, r);
}

// the lines of text as getline returns them: each with its '\n', the last one also without (a NUL inside a line ends it for
// the parser, as it does after getline)
static void feed_text(dsb_report *R, const char *text, size_t len)
{
	for (size_t a = 0; a < len;) {
		const char *e = (const char *)memchr(text + a, '\n', len - a);
		const size_t b = e ? (size_t)(e - text) + 1 : len;
		R->line.assign(text + a, b - a); feed_line(R, &R->line[0]);
		a = b;
	}
}

extern "C" int dsb_report_create(const dsb_taxonomy *T, dsb_report **out)
{
	if (!T || !out) return DSB_EINVAL;
	dsb_report *R = new (std::nothrow) dsb_report();
	if (!R) return DSB_ENOMEM;
	R->T = T;
	try { R->count.assign((size_t)T->max_tid + 1, 0); R->base.assign((size_t)T->max_tid + 1, 0); R->mq.assign((size_t)T->max_tid + 1, 0); }
	catch (...) { delete R; return DSB_ENOMEM; }
	*out = R;
	return DSB_OK;
}
extern "C" void dsb_report_destroy(dsb_report *R) { delete R; }

extern "C" int dsb_report_add_sam(dsb_report *R, const char *text, size_t len)
{
	if (!R || (!text && len)) return DSB_EINVAL;
	feed_text(R, text, len);
	return DSB_OK;
}

// a name the SAM text gives back as it is (the first tab-separated field of a line that is not taken for a header line)
static bool plain_name(const char *s) { return s[0] && s[0] != '@' && !strpbrk(s, "\t\n"); }

// the records dsb_format_sam prints for one read (without SEQ / QUAL: they do not reach the report), fed line by line
static int feed_read_host(dsb_report *R, const dsb_index *idx, const dsb_read *rd, const dsb_hit *h, uint32_t n, int max_sec)
{
	const size_t need = 4096 + 800 * (size_t)n + strlen(rd->name) * (n + 1);
	if (R->sam.size() < need) R->sam.resize(need);
	const long w = dsb_format_sam(idx, rd, h, n, max_sec, 0, R->sam.data(), R->sam.size());
	if (w < 0) return DSB_ENOMEM;
	feed_text(R, R->sam.data(), (size_t)w);
	return DSB_OK;
}

extern "C" int dsb_report_add(dsb_report *R, const dsb_index *idx, const dsb_read *reads, const dsb_result *res, const dsb_read_taxon *taxa, size_t n, int max_sec)
{
	if (!R || !idx || (n && (!reads || !res || !res->reads))) return DSB_EINVAL;
	for (size_t i = 0; i < n; i++) {
		const dsb_read_result &rr = res->reads[i];
		const dsb_read &rd = reads[i];
		const dsb_hit *h = rr.n ? res->hits + rr.first : NULL;
		if (taxa && !(taxa[i].flags & DSB_TAXON_HOST) && plain_name(rd.name) && !(R->open && R->name == rd.name)) {
			const dsb_read_taxon &t = taxa[i];
			if (R->open) close_read(R);
			R->head = false;
			start_read(R, rd.name, (t.flags & DSB_TAXON_CLASSIFIED) ? 'C' : 'U', t.taxid, t.score, t.len, t.mapq);
			continue;
		}
		int rc = feed_read_host(R, idx, &rd, h, rr.n, max_sec);
		if (rc) return rc;
	}
	return DSB_OK;
}

uint32_t dsb_read_taxid_host(const dsb_taxonomy *T, const dsb_index *idx, uint32_t read_len, const dsb_hit *h, uint32_t n, int max_sec)
{
	// the read's own records through a report of its own; the read it leaves open is the answer
	dsb_report R; R.T = T;
	dsb_read rd; rd.name = "r"; rd.seq = ""; rd.qual = NULL; rd.len = read_len;
	std::vector<char> buf(4096 + 800 * (size_t)n);
	const long w = dsb_format_sam(idx, &rd, h, n, max_sec, 0, buf.data(), buf.size());
	if (w <= 0) return 0;
	std::string line(buf.data(), (size_t)w);
	char *s = &line[0];
	const char *e = strchr(s, '\n');
	Rec first;
	std::string l0(s, e ? (size_t)(e - s + 1) : strlen(s));
	if (parse_sam_line(&l0[0], &first) || first.cls != 'C' || first.tid > T->max_tid) return 0;
	uint32_t tid = first.tid;
	if (first.score == 0) return tid;
	for (const char *p = e ? e + 1 : NULL; p && *p;) {
		const char *q = strchr(p, '\n');
		std::string l(p, q ? (size_t)(q - p + 1) : strlen(p));
		p = q ? q + 1 : NULL;
		Rec r;
		if (parse_sam_line(&l[0], &r) || strcmp(r.name, "r") != 0) continue;
		if (r.score != first.score || r.tid > T->max_tid) continue;
		if (descends(T, r.tid, tid)) tid = r.tid;
	}
	return tid;
}

// ---- the printout ----
struct Kid { uint32_t tid, next; };
struct Node { uint64_t weight; uint32_t first_kid; uint64_t mapq_sum; };
struct ByCount { uint32_t tid; int count; };                         // COUNT_SORT, src/analysis.c:1260-1263
struct ByBase { uint32_t tid; uint64_t base, map_q; };               // NODE_BASE_Q, src/analysis.c:1610-1614
static int less_count(const void *a, const void *b) { return ((const ByCount *)a)->count < ((const ByCount *)b)->count; }
static int less_base(const void *a, const void *b) { return ((const ByBase *)a)->base < ((const ByBase *)b)->base; }

// add `w` (and `q`) to tid and all its ancestors; remember each parent -> child edge once, in order of first use
static void add_up(const dsb_taxonomy *T, Node *N, Kid *K, uint32_t *n_kid, uint32_t tid, uint64_t w, uint64_t q)
{
	N[tid].weight += w; N[tid].mapq_sum += q;
	for (uint32_t c = tid;;) {
		const uint32_t p = T->parent[c];
		if (p < 1 || p == DSB_TID_NONE || p >= T->max_tid) break;
		N[p].weight += w; N[p].mapq_sum += q;
		if (N[p].first_kid == 0) { N[p].first_kid = (*n_kid)++; K[N[p].first_kid].tid = c; }
		else {
			uint32_t k = N[p].first_kid;
			while (K[k].tid != c && K[k].next != 0) k = K[k].next;
			if (K[k].tid != c) { K[k].next = (*n_kid)++; K[K[k].next].tid = c; }
		}
		c = p;
	}
}

static void put(std::string &o, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
static void put(std::string &o, const char *fmt, ...)
{
	char b[512]; va_list ap; va_start(ap, fmt);
	int w = vsnprintf(b, sizeof b, fmt, ap); va_end(ap);
	if (w > 0) o.append(b, (size_t)w < sizeof b ? (size_t)w : sizeof b - 1);
}

static void print_tree(std::string &o, const dsb_taxonomy *T, const Node *N, const Kid *K, uint32_t id, int depth, uint64_t total, int with_mapq)
{
	const float rate = (float)N[id].weight / total * 100;
	const float map_q = (float)N[id].mapq_sum / N[id].weight * rate;
	if (rate < 0.01) return;
	o.append((size_t)depth, '|');
	if (with_mapq) put(o, "%s TID:%d %s %f%%, mapQ:%f\n", T->rank[id], id, "", rate, map_q);
	else put(o, "%s TID:%d %s %f%%\n", T->rank[id], id, "", rate);
	for (uint32_t k = N[id].first_kid; k != 0; k = K[k].next) print_tree(o, T, N, K, K[k].tid, depth + 1, total, with_mapq);
}

extern "C" long dsb_report_format(const dsb_report *R, int by_base, char *buf, size_t cap)
{
	if (!R) return -1;
	std::string o;
	if (R->any) {
		const dsb_taxonomy *T = R->T; const uint32_t max_tid = T->max_tid;
		std::vector<Node> N((size_t)max_tid + 1, Node{0, 0, 0});
		std::vector<Kid> K(2 * (size_t)max_tid + 2, Kid{0, 0});
		uint32_t n_kid = 1;
		if (!by_base) {
			std::vector<ByCount> s; s.reserve(1024);
			for (uint32_t t = 0; t <= max_tid; t++) if (R->count[t]) s.push_back(ByCount{t, (int)R->count[t]});
			qsort(s.data(), s.size(), sizeof(ByCount), less_count);
			for (const ByCount &e : s) add_up(T, N.data(), K.data(), &n_kid, e.tid, R->count[e.tid], 0);
			o += "Data:\n";
			print_tree(o, T, N.data(), K.data(), 1, 0, (uint64_t)R->total_reads, 0);
			put(o, "total_read_number :%d\t", R->total_reads);
		} else {
			std::vector<ByBase> s; s.reserve(1024);
			for (uint32_t t = 0; t <= max_tid; t++) if (R->base[t]) s.push_back(ByBase{t, R->base[t], R->mq[t]});
			qsort(s.data(), s.size(), sizeof(ByBase), less_base);
			for (const ByBase &e : s) add_up(T, N.data(), K.data(), &n_kid, e.tid, R->base[e.tid], R->mq[e.tid]);
			o += "Analysis based on base number:\n";
			print_tree(o, T, N.data(), K.data(), 1, 0, R->total_base, 1);
			put(o, "total_mapped_base_number :%ld\n", (long)R->total_base);
			put(o, "low identity read (identity <= 75%%) number :%ld\t", (long)R->low_n);
			put(o, "total base %ld\t", (long)R->low_base);
		}
	}
	if (!buf || o.size() >= cap) return -1;
	memcpy(buf, o.data(), o.size()); buf[o.size()] = 0;
	return (long)o.size();
}

// ---- the per-reference abundance table: fixed formats, so that equal doubles give equal text ----
extern "C" long dsb_abundance_format(const dsb_index *x, const dsb_ref_abundance *ab, const dsb_abundance_summary *sum, char *buf, size_t cap)
{
	if (!x || !ab || !sum || (!buf && cap)) return -1;
	size_t o = 0; int w;
#define EMIT(...) do { w = snprintf(buf + o, cap > o ? cap - o : 0, __VA_ARGS__); if (w < 0 || (size_t)w >= (cap > o ? cap - o : 0)) return -1; o += (size_t)w; } while (0)
	EMIT("#reads=%llu\tclassified=%llu\tclasses=%llu\titerations=%u\tconverged=%s\tmax_change=%.6e\tmin_frac=%.3f\n", (unsigned long long)sum->reads,
	     (unsigned long long)sum->classified, (unsigned long long)sum->classes, sum->iterations, sum->converged ? "yes" : "no", sum->max_change,
	     sum->min_permille / 1000.0);
	EMIT("#rname\ttaxid\tlength\tnumreads\tuniqreads\testreads\treadshare\tcopyshare\n");
	const uint64_t n_ref = dsb_index_n_ref(x);
	for (uint64_t r = 0; r < n_ref; r++) {
		const dsb_ref_abundance &a = ab[r];
		if (!a.numreads) continue;
		const char *name = dsb_index_ref_name(x, (uint32_t)r);
		const uint32_t tid = dsb_ref_taxid(name);
		EMIT("%s\t%u\t%llu\t%llu\t%llu\t%.3f\t%.6e\t%.6e\n", name, tid == DSB_TID_NONE ? 0u : tid, (unsigned long long)dsb_index_ref_len(x, (uint32_t)r),
		     (unsigned long long)a.numreads, (unsigned long long)a.uniqreads, a.est_reads, a.read_share, a.copy_share);
	}
#undef EMIT
	return (long)o;
}

// one read's line of the per-read assignment
extern "C" long dsb_format_assign(const dsb_index *x, const dsb_read *rd, const dsb_read_assign *a, char *buf, size_t cap)
{
	if (!x || !rd || !rd->name || !a || !buf) return -1;
	int w;
	if (a->ref_ID == DSB_ASSIGN_NONE) w = snprintf(buf, cap, "%s\t*\t0\t0\t0.000000\n", rd->name);
	else {
		if (a->ref_ID >= dsb_index_n_ref(x)) return -1;
		const char *name = dsb_index_ref_name(x, a->ref_ID);
		const uint32_t tid = dsb_ref_taxid(name);
		w = snprintf(buf, cap, "%s\t%s\t%u\t%u\t%.6f\n", rd->name, name, tid == DSB_TID_NONE ? 0u : tid, a->n_cand, a->posterior);
	}
	return (w < 0 || (size_t)w >= cap) ? -1 : (long)w;
}

// ---- names.dmp, Kraken's per-read line and Kraken's report for the LCA classification ----
extern "C" int dsb_taxnames_load(const char *path, dsb_taxnames **out)
{
	if (!path || !out) return DSB_EINVAL;
	FILE *f = fopen(path, "r");
	if (!f) return DSB_EIO;
	dsb_taxnames *N = new dsb_taxnames;
	std::vector<std::pair<uint32_t, std::string>> rows;
	char *line = NULL; size_t m = 0;
	while (getline(&line, &m, f) > 0) {
		// taxid \t|\t name \t|\t unique name \t|\t name class \t|
		std::string fld[4]; int k = 0;
		for (const char *s = line; k < 4;) {
			const char *e = strstr(s, "\t|");
			if (!e) break;
			fld[k++].assign(s, (size_t)(e - s));
			s = e + 2; if (*s == '\t') s++;
		}
		if (k < 4 || fld[3] != "scientific name" || fld[0].empty()) continue;
		rows.emplace_back((uint32_t)strtoul(fld[0].c_str(), NULL, 10), fld[1]);
	}
	free(line); fclose(f);
	std::stable_sort(rows.begin(), rows.end(), [](const std::pair<uint32_t, std::string> &a, const std::pair<uint32_t, std::string> &b) { return a.first < b.first; });
	for (const auto &r : rows) if (N->tid.empty() || N->tid.back() != r.first) { N->tid.push_back(r.first); N->name.push_back(r.second); }   // (the first of a taxid's lines)
	*out = N;
	return DSB_OK;
}
extern "C" void dsb_taxnames_close(dsb_taxnames *N) { delete N; }

extern "C" long dsb_format_kraken(const dsb_read *rd, const dsb_read_lca *l, char *buf, size_t cap)
{
	if (!rd || !rd->name || !l || !buf) return -1;
	const int w = snprintf(buf, cap, "%c\t%s\t%u\t%u\t%u:%u\n", l->taxid ? 'C' : 'U', rd->name, l->taxid, rd->len, l->score, l->n_pass);
	return (w < 0 || (size_t)w >= cap) ? -1 : (long)w;
}

// the letter of a rank that has one in Kraken's report, else 0
static char rank_letter(const char *r)
{
	static const struct { const char *rank; char c; } tab[] = {{"superkingdom", 'D'}, {"domain", 'D'}, {"kingdom", 'K'}, {"phylum", 'P'}, {"class", 'C'},
	                                                           {"order", 'O'}, {"family", 'F'}, {"genus", 'G'}, {"species", 'S'}};
	for (const auto &e : tab) if (!strcmp(r, e.rank)) return e.c;
	return 0;
}

extern "C" long dsb_lca_report_format(const dsb_taxonomy *T, const dsb_taxnames *names, const dsb_taxon_count *rows, size_t n, const dsb_lca_summary *sum,
                                      char *buf, size_t cap)
{
	if (!T || !sum || (!rows && n) || !buf) return -1;
	std::string o;
	if (sum->reads) {
		const double reads = (double)sum->reads;
		if (sum->reads > sum->classified) {
			const unsigned long long u = sum->reads - sum->classified;
			put(o, "%6.2f\t%llu\t%llu\tU\t0\tunclassified\n", 100.0 * (double)u / reads, u, u);
		}
		// the rows by taxid (they come ascending from dsb_ctx_lca_counts; hand-filled ones need not), the children of each
		std::vector<uint32_t> by(n);
		for (size_t i = 0; i < n; i++) by[i] = (uint32_t)i;
		std::sort(by.begin(), by.end(), [&](uint32_t a, uint32_t b) { return rows[a].taxid < rows[b].taxid; });
		auto find = [&](uint32_t tid) -> long {
			size_t lo = 0, hi = n;
			while (lo < hi) { const size_t mid = (lo + hi) / 2; if (rows[by[mid]].taxid < tid) lo = mid + 1; else hi = mid; }
			return lo < n && rows[by[lo]].taxid == tid ? (long)lo : -1;
		};
		std::vector<std::vector<uint32_t>> kids(n);              // (positions in `by`)
		for (size_t k = 0; k < n; k++) {
			const dsb_taxon_count &r = rows[by[k]];
			if (!r.clade_reads || r.taxid <= 1 || r.taxid > T->max_tid) continue;
			const long p = find(T->parent[r.taxid]);
			if (p >= 0) kids[(size_t)p].push_back((uint32_t)k);
		}
		for (auto &v : kids)
			std::sort(v.begin(), v.end(), [&](uint32_t a, uint32_t b) {
				const dsb_taxon_count &x = rows[by[a]], &y = rows[by[b]];
				return x.clade_reads != y.clade_reads ? x.clade_reads > y.clade_reads : x.taxid < y.taxid;
			});
		struct Frame { uint32_t k, depth, num; char letter; };
		std::vector<Frame> st;
		const long root = find(1);
		if (root >= 0 && rows[by[(size_t)root]].clade_reads) st.push_back(Frame{(uint32_t)root, 0, 0, 'R'});
		while (!st.empty()) {
			const Frame f = st.back(); st.pop_back();
			const dsb_taxon_count &r = rows[by[f.k]];
			put(o, "%6.2f\t%llu\t%llu\t%c", 100.0 * (double)r.clade_reads / reads, (unsigned long long)r.clade_reads, (unsigned long long)r.direct_reads, f.letter);
			if (f.num) put(o, "%u", f.num);
			put(o, "\t%u\t%*s", r.taxid, (int)(2 * f.depth), "");
			const std::string *nm = nullptr;
			if (names) { auto it = std::lower_bound(names->tid.begin(), names->tid.end(), r.taxid); if (it != names->tid.end() && *it == r.taxid) nm = &names->name[(size_t)(it - names->tid.begin())]; }
			if (nm) { o += *nm; o += '\n'; } else put(o, "%u\n", r.taxid);
			const std::vector<uint32_t> &v = kids[f.k];
			for (size_t j = v.size(); j-- > 0;) {                   // (pushed in reverse: the first child is printed first)
				const char c = rank_letter(T->rank[rows[by[v[j]]].taxid]);
				st.push_back(c ? Frame{v[j], f.depth + 1, 0, c} : Frame{v[j], f.depth + 1, f.num + 1, f.letter});
			}
		}
	}
	if (o.size() >= cap) return -1;
	memcpy(buf, o.data(), o.size()); buf[o.size()] = 0;
	return (long)o.size();
}
