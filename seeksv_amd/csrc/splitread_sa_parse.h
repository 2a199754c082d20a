// splitread_sa_parse.h - `seeksv run -A -S`: the byte work on a record's optional fields (the rule: include/seeksv_hip.h at ssv_rt_begin_original_sa;
// DESIGN.md 8h).  Two walkers that find the value of the first SA:Z field - one over BAM's typed fields, one over SAM text - the parser of that value's first
// entry, the geometry k_sr_gather would give a record of that entry, and the contig look-up.  Everything works on (p, end) and never reads at or beyond end.
// __host__ __device__ and free of HIP: the kernels (splitread_sa_kernels.h) and a stand-alone CPU program (tests/native/sa_parse_check.cpp) compile the same text.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define SSV_HD __host__ __device__ __forceinline__
#else
#define SSV_HD inline
#endif

namespace ssv {

enum : int { SA_OK = 0, SA_REFUSED = 1, SA_MULTI = 2 };
enum : int { SA_ENC_BAM = 0, SA_ENC_SAM = 1 };

// BAM's typed fields (A c C s S i I f d Z H B, as aux_xc_flag walks them): the value of the first field with tag SA and type Z -> [*vb, *ve) without its NUL.
// An unknown type ends the walk; a Z / H without a NUL before end, a B array or a fixed-size value that runs over end: no value.
SSV_HD bool sa_find_bam(const uint8_t *p, const uint8_t *end, const uint8_t **vb, const uint8_t **ve)
{
	while (end - p >= 3) {
		const uint8_t t0 = p[0], t1 = p[1], ty = p[2];
		p += 3;
		uint64_t sz;
		switch (ty) {
		case 'A': case 'c': case 'C': sz = 1; break;
		case 's': case 'S': sz = 2; break;
		case 'i': case 'I': case 'f': sz = 4; break;
		case 'd': sz = 8; break;
		case 'Z': case 'H': {
			const uint8_t *q = p;
			while (q < end && *q) ++q;
			if (q == end) return false;
			if (ty == 'Z' && t0 == 'S' && t1 == 'A') { *vb = p; *ve = q; return true; }
			sz = (uint64_t)(q - p) + 1;
			break;
		}
		case 'B': {
			if (end - p < 5) return false;
			const uint8_t st = p[0];
			const uint64_t cnt = (uint64_t)p[1] | (uint64_t)p[2] << 8 | (uint64_t)p[3] << 16 | (uint64_t)p[4] << 24;
			sz = 5 + cnt * ((st == 'c' || st == 'C') ? 1u : (st == 's' || st == 'S') ? 2u : 4u);
			break;
		}
		default: return false;
		}
		if ((uint64_t)(end - p) < sz) return false;
		p += sz;
	}
	return false;
}

// SAM text from the start of field 12: the value of the first field that begins with "SA:Z:" -> [*vb, *ve).  A field ends at a tab, at a newline (a '\r'
// right in front of it is not part of the value) or at end.
SSV_HD bool sa_find_sam(const uint8_t *p, const uint8_t *end, const uint8_t **vb, const uint8_t **ve)
{
	while (p < end) {
		const uint8_t *q = p;
		while (q < end && *q != '\t' && *q != '\n') ++q;
		if (q - p >= 5 && p[0] == 'S' && p[1] == 'A' && p[2] == ':' && p[3] == 'Z' && p[4] == ':') {
			const uint8_t *e = q;
			if (q < end && *q == '\n' && e > p + 5 && e[-1] == '\r') --e;
			*vb = p + 5; *ve = e;
			return true;
		}
		if (q == end || *q == '\n') return false;
		p = q + 1;
	}
	return false;
}

// one entry of an SA value, and what its CIGAR says (lengths as sr_shape and k_sr_gather take them from a record's operations; S and H are both clips)
struct SaEntry {
	const uint8_t *rname; uint32_t rname_len;
	const uint8_t *cigar; uint32_t cigar_len; // the CIGAR's text
	int32_t pos0;                             // pos - 1
	int32_t mapq;
	uint8_t strand;                           // '+' / '-'
	bool first_clip, last_clip;
	uint32_t n_ops, n_keep;                   // operations; those that are no clips
	int64_t R;                                // M I S = X H
	int64_t clip_front, clip_back;            // the runs of clips at the two ends
	uint32_t ref_len;                         // M D = N (32 bits, wrapping as k_sr_gather's int does)
};

SSV_HD int sa_cigar_code(uint8_t ch)
{
	switch (ch) {
	case 'M': return 0; case 'I': return 1; case 'D': return 2; case 'N': return 3; case 'S': return 4;
	case 'H': return 5; case 'P': return 6; case '=': return 7; case 'X': return 8; default: return -1;
	}
}

// decimal digits at *pp up to `max`: at least one digit, no sign; *pp moves behind them
SSV_HD bool sa_number(const uint8_t **pp, const uint8_t *end, uint64_t max, uint64_t *out)
{
	const uint8_t *p = *pp;
	uint64_t v = 0;
	bool any = false;
	while (p < end && *p >= '0' && *p <= '9') {
		v = v * 10 + (uint64_t)(*p - '0');
		if (v > max) return false;
		any = true;
		++p;
	}
	*pp = p; *out = v;
	return any;
}

// the next operation of a CIGAR text that sa_parse_entry accepted: BAM's encoding (length << 4 | code)
SSV_HD uint32_t sa_cigar_next(const uint8_t **pp)
{
	const uint8_t *p = *pp;
	uint32_t v = 0;
	while (*p >= '0' && *p <= '9') v = v * 10 + (uint32_t)(*p++ - '0');
	const uint32_t op = (uint32_t)sa_cigar_code(*p++);
	*pp = p;
	return v << 4 | op;
}

// rname,pos,strand,CIGAR,mapQ,NM; as written: SA_OK with *o filled, SA_MULTI when bytes follow the entry's ';', SA_REFUSED for anything else
SSV_HD int sa_parse_entry(const uint8_t *p, const uint8_t *end, SaEntry *o)
{
	uint64_t v;
	o->rname = p;
	while (p < end && *p != ',') ++p;
	if (p == end) return SA_REFUSED;
	o->rname_len = (uint32_t)(p - o->rname);
	++p;
	if (!sa_number(&p, end, 0x7fffffffull, &v) || v < 1 || p == end || *p != ',') return SA_REFUSED;
	o->pos0 = (int32_t)(v - 1);
	++p;
	if (p == end || (*p != '+' && *p != '-')) return SA_REFUSED;
	o->strand = *p++;
	if (p == end || *p != ',') return SA_REFUSED;
	++p;
	o->cigar = p;
	o->n_ops = o->n_keep = 0; o->R = 0; o->clip_front = o->clip_back = 0; o->ref_len = 0;
	o->first_clip = o->last_clip = false;
	while (p < end && *p != ',') {
		if (!sa_number(&p, end, (1ull << 28) - 1, &v) || p == end) return SA_REFUSED;
		const int op = sa_cigar_code(*p);
		if (op < 0) return SA_REFUSED;
		++p;
		if (++o->n_ops > 65535u) return SA_REFUSED;
		const bool clip = op == 4 || op == 5;
		if (op == 0 || op == 1 || op == 4 || op == 7 || op == 8 || op == 5) o->R += (int64_t)v;
		if (op == 0 || op == 2 || op == 7 || op == 3) o->ref_len += (uint32_t)v;
		if (o->n_ops == 1) o->first_clip = clip;
		o->last_clip = clip;
		if (clip) { if (!o->n_keep) o->clip_front += (int64_t)v; o->clip_back += (int64_t)v; }
		else { ++o->n_keep; o->clip_back = 0; }
	}
	if (p == end || o->n_ops == 0) return SA_REFUSED;
	o->cigar_len = (uint32_t)(p - o->cigar);
	++p;
	if (!sa_number(&p, end, 255, &v) || p == end || *p != ',') return SA_REFUSED;
	o->mapq = (int32_t)v;
	++p;
	const uint8_t *const nm = p; // NM: a run of digits (at least one), not read
	while (p < end && *p >= '0' && *p <= '9') ++p;
	if (p == nm) return SA_REFUSED;
	if (p == end) return SA_OK;        // (a missing final ';' at the value's end)
	if (*p != ';') return SA_REFUSED;
	return p + 1 == end ? SA_OK : SA_MULTI;
}

// the candidate fields of an accepted entry, by k_sr_gather's formulas.  false: not exactly one end is clipped.
struct SaGeometry { int32_t pos, lq, left, right; uint8_t side; };
SSV_HD bool sa_geometry(const SaEntry &e, SaGeometry *g)
{
	if (e.first_clip == e.last_clip) return false;
	const int R = e.R > 0x3fffffff ? -1 : (int)e.R;
	g->lq = R;
	if (e.first_clip) { const int clip = (int)e.clip_front; g->side = '5'; g->left = clip; g->right = R - clip; g->pos = e.pos0 + 1; }
	else { const int clip = (int)e.clip_back; g->side = '3'; g->right = clip; g->left = R - clip; g->pos = (int32_t)((uint32_t)e.pos0 + e.ref_len); }
	return true;
}

// The header's contigs for the look-up of an rname: FNV-1a hashes (cut to `mask`) sorted with their tids, and the names' bytes one behind the other
// (name t: names[name_off[t] .. name_off[t + 1])).  Names that share a hash lie side by side and are told apart by their bytes.
struct SaContigs { const uint64_t *hash; const uint32_t *tid; const uint64_t *name_off; const uint8_t *names; int64_t n; uint64_t mask; };

SSV_HD uint64_t sa_name_hash(const uint8_t *s, uint32_t len)
{
	uint64_t h = 1469598103934665603ull;
	for (uint32_t j = 0; j < len; ++j) h = (h ^ s[j]) * 1099511628211ull;
	return h;
}

SSV_HD int32_t sa_contig_find(const SaContigs &T, const uint8_t *s, uint32_t len)
{
	const uint64_t h = sa_name_hash(s, len) & T.mask;
	int64_t lo = 0, hi = T.n;
	while (lo < hi) { const int64_t mid = lo + (hi - lo) / 2; if (T.hash[mid] < h) lo = mid + 1; else hi = mid; }
	for (int64_t k = lo; k < T.n && T.hash[k] == h; ++k) {
		const uint32_t t = T.tid[k];
		const uint64_t o = T.name_off[t];
		if (T.name_off[t + 1] - o != len) continue;
		uint32_t j = 0;
		while (j < len && T.names[o + j] == s[j]) ++j;
		if (j == len) return (int32_t)t;
	}
	return -1;
}

// a source's optional fields -> its entry: SA_OK / SA_REFUSED / SA_MULTI, or -1 when there is no SA:Z field
SSV_HD int sa_entry_of(const uint8_t *p, const uint8_t *end, int enc, SaEntry *e)
{
	const uint8_t *vb, *ve;
	if (!(enc == SA_ENC_SAM ? sa_find_sam(p, end, &vb, &ve) : sa_find_bam(p, end, &vb, &ve))) return -1;
	return sa_parse_entry(vb, ve, e);
}

} // namespace ssv
