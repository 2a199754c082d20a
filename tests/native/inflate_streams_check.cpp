// CPU check of seeksv_amd/csrc/inflate_core.h against the catalogue of hand-written DEFLATE streams (tests/deflate_cases.py): streams no compressor writes -
// codes longer than any look-up table, distances up to 32,768, both encodings of length 258, blocks at every bit phase, empty blocks - and malformed ones.
// Built and run by tests/test_deflate_cases.py, once plain and once with -fsanitize=address,undefined.
//   usage: inflate_streams_check FILE [dist]       (dist: also print the largest match distance among all valid streams' tokens)
//   FILE:  u32 count, then per case: u32 name length, name, u32 valid, u32 input bytes, u32 output bytes (the ISIZE the container claims), the input,
//          and for a valid case the bytes it inflates to
// Every case goes through the decoder's three forms: DirectOut / PlainTab; TokenOut / PlainTabLim + resolve_tokens at four output misalignments; RingReader at
// four input misalignments.  A valid case must give its bytes, leave the guard bytes on both sides of the output alone and need at most token_capacity tokens;
// a malformed one must be refused by every form.  Exit code 0 = all of that held.
#include <stdio.h>
#include <stdlib.h>
#include <string>
#include <vector>

#include "inflate_core.h"

struct CpuRing {
	uint32_t a[32];
	uint32_t get(uint32_t j) const { return a[j]; }
	void set(uint32_t j, uint32_t v) { a[j] = v; }
	bool any(bool c) const { return c; }
};

static bool rd32(FILE *f, uint32_t &v) { return fread(&v, 4, 1, f) == 1; }

static bool guards(const std::vector<uint8_t> &buf, size_t front, size_t n)
{
	for (size_t g = 0; g < front; ++g) if (buf[g] != 0x55) return false;
	for (size_t g = front + n; g < buf.size(); ++g) if (buf[g] != 0x55) return false;
	return true;
}

int main(int argc, char **argv)
{
	if (argc != 2 && argc != 3) { fprintf(stderr, "usage: %s FILE [dist]\n", argv[0]); return 2; }
	uint32_t max_dist = 0;
	FILE *f = fopen(argv[1], "rb");
	if (!f) { perror(argv[1]); return 2; }
	uint32_t count = 0;
	if (!rd32(f, count)) return 2;
	int n_valid = 0, n_refused = 0, n_bad = 0;
	ssv::PlainTab tab;
	ssv::PlainTabLim tabl;
	for (uint32_t ci = 0; ci < count; ++ci) {
		uint32_t nl, valid, clen, n;
		if (!rd32(f, nl)) return 2;
		std::string name(nl, ' ');
		if (nl && fread(&name[0], 1, nl, f) != nl) return 2;
		if (!rd32(f, valid) || !rd32(f, clen) || !rd32(f, n)) return 2;
		std::vector<uint8_t> c((size_t)clen + 40, 0xAA), want(n);
		if (clen && fread(c.data(), 1, clen, f) != clen) return 2;
		if (valid && n && fread(want.data(), 1, n, f) != n) return 2;
		want.reserve(n + 1);
		const uint32_t cap = ssv::token_capacity(n);
		int fails = 0;
		auto verdict = [&](const char *form, int mis, int rc, bool bytes_ok, bool guard_ok, bool tok_ok) {
			if (valid) {
				if (rc != ssv::INF_OK || !bytes_ok || !guard_ok || !tok_ok) { ++fails; fprintf(stderr, "%s: %s (misalignment %d): rc %d bytes %d guards %d tokens %d\n", name.c_str(), form, mis, rc, (int)bytes_ok, (int)guard_ok, (int)tok_ok); }
			} else if (rc == ssv::INF_OK || !guard_ok || !tok_ok) { ++fails; fprintf(stderr, "%s: %s (misalignment %d): malformed stream: rc %d guards %d tokens %d\n", name.c_str(), form, mis, rc, (int)guard_ok, (int)tok_ok); }
		};
		{ // straight into the output
			std::vector<uint8_t> o((size_t)n + 32, 0x55);
			const int rc = ssv::inflate_stream(c.data(), clen, o.data() + 16, n, tab);
			verdict("direct", 0, rc, !valid || memcmp(o.data() + 16, want.data(), n) == 0, guards(o, 16, n), true);
		}
		for (int mo = 0; mo < 4; ++mo) { // tokens, then the holes filled in order; the output at every misalignment
			std::vector<uint8_t> o((size_t)n + 40, 0x55);
			uint8_t *op = o.data() + 16 + mo;
			std::vector<uint32_t> tk((size_t)cap + 1, 0xdeadbeefu);
			ssv::TokenOut to;
			to.out = op; to.tok = tk.data();
			const int rc = ssv::inflate_stream_to(c.data(), clen, to, n, tabl);
			const bool tok_ok = to.n <= cap && tk[cap] == 0xdeadbeefu;
			if (rc == ssv::INF_OK && tok_ok) ssv::resolve_tokens(op, tk.data(), to.n);
			if (rc == ssv::INF_OK && tok_ok && valid && mo == 0)
				for (uint32_t t = 0; t < to.n; ++t) if ((tk[t] >> 23) != 511u) { const uint32_t dist = ((tk[t] >> 8) & 0x7fffu) + 1u; if (dist > max_dist) max_dist = dist; }
			verdict("tokens", mo, rc, !valid || memcmp(op, want.data(), n) == 0, guards(o, 16 + (size_t)mo, n), tok_ok);
		}
		for (int mi = 0; mi < 4; ++mi) { // the window reader in front of the token sink, the input at every misalignment
			std::vector<uint8_t> cc((size_t)clen + 4 + 40, 0xAA);
			memcpy(cc.data() + mi, c.data(), clen);
			std::vector<uint8_t> o((size_t)n + 32, 0x55);
			std::vector<uint32_t> tk((size_t)cap + 1, 0xdeadbeefu);
			ssv::TokenOut to;
			to.out = o.data() + 16; to.tok = tk.data();
			int rc;
			if (mi & 1) { ssv::RingReader<CpuRing, 64> br(cc.data() + mi, clen, CpuRing()); rc = ssv::inflate_stream_from(br, cc.data() + mi, clen, to, n, tab); }
			else { ssv::RingReader<CpuRing, 128> br(cc.data() + mi, clen, CpuRing()); rc = ssv::inflate_stream_from(br, cc.data() + mi, clen, to, n, tabl); }
			const bool tok_ok = to.n <= cap && tk[cap] == 0xdeadbeefu;
			if (rc == ssv::INF_OK && tok_ok) ssv::resolve_tokens(o.data() + 16, tk.data(), to.n);
			verdict("ring", mi, rc, !valid || memcmp(o.data() + 16, want.data(), n) == 0, guards(o, 16, n), tok_ok);
		}
		if (fails) ++n_bad;
		else if (valid) ++n_valid;
		else ++n_refused;
	}
	fclose(f);
	if (argc == 3) printf("largest match distance %u\n", max_dist);
	printf("%d valid streams decoded, %d malformed streams refused, %d bad\n", n_valid, n_refused, n_bad);
	return n_bad ? 1 : 0;
}
