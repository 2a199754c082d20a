// seeksv_cli.cpp - the `seeksv` command line on top of libseeksv_host (BAM decoding, getsv bookkeeping) and
// libseeksv_hip (HIP kernels).  Keeps the reference's sub-commands, flags, defaults, file names, output columns and
// stderr / stdout messages for the hot path (seeksv.cpp:128-155 CallGetclip, :157-330 CallGetsv):
//
//   seeksv getclip [-t f] [-q n] [-s] [-o prefix] in.sorted.bam
//   seeksv getsv   [options] clip.bam in.sorted.bam clip.gz out.sv out.unmapped.clip.fq
//   seeksv run     [-P] [-N n [-G d0,d1,...]] [-c "getclip options"] [-v "getsv options"] [-a "realign options"] in.sorted.bam ref.fa prefix
//                  (getclip, realign and getsv in one process, one decode; -P: the unmapped pairs split-aligned on the way and handed to the -F pass
//                  as a device batch - run_split_leg, ssv_realign_split_batch; -N: the decode and the records over n GPUs - RunRanks, ranks_tally)
//
// getsv: junctions come from `-B <table>` (ReadBreakpoint, getsv.cpp:1292) and / or from the join of clip.gz with clip.bam
// (junction_stage.cpp); the BAM passes run on the GPU; OutputBreakpoint's filter chain and columns are reproduced here.
// No .bai is needed: the discordant pass scans the BAM instead of seeking in it.
#include <getopt.h>
#include <zlib.h>

#include <algorithm>
#include <array>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <functional>
#include <iostream>
#include <deque>
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <dirent.h>
#include <pthread.h>
#include <sys/resource.h>
#include <unistd.h>
#include <atomic>
#include "../csrc/cpus.h"
#include <condition_variable>
#include <map>
#include <mutex>
#include <shared_mutex>
#include <sstream>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "junction_stage.h"
#include "readthrough_stage.h"
#include "sam_text.h"
#include "somatic_stage.h"
#include "unmapped_pairs.h"
#include "fastq_reads.h"
#include "regions.h"
#include "../csrc/thp.h"
#include "seeksv_hip.h"
#include "seeksv_host.h"

using namespace std;
using seeksv::Junction;
using seeksv::JunctionMap;
using seeksv::OtherInfo;
using seeksv::SeqInfo;
using seeksv::parse_cigar;
using seeksv::NormalClusters;
using seeksv::SomaticRow;
using seeksv::load_normal_clusters;
using seeksv::parse_tumor_table;
using seeksv::probe_normal_clusters;
using seeksv::scan_tumor_table;

static const char *kVersion = "1.2.3-mi355x";

// SSV_TIMING=1: wall time of the phases on stderr
struct PhaseTimer {
	bool on = getenv("SSV_TIMING") != nullptr;
	std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
	std::map<std::string, double> acc;
	std::vector<std::string> order;
	void lap(const char *name)
	{
		if (!on) return;
		auto t1 = std::chrono::steady_clock::now();
		if (!acc.count(name)) order.push_back(name);
		acc[name] += std::chrono::duration<double>(t1 - t0).count();
		t0 = t1;
	}
	~PhaseTimer() { if (on) for (auto &n : order) std::cerr << "[timing] " << n << " " << acc[n] << " s" << std::endl; }
};

// A fatal error: the reference's message and exit status 1.  Reader, emitter and rank threads may be running (and the HIP context coming up on its own
// thread): the process leaves through _exit - no static destructor pulls a buffer away under a thread that is still copying into it - after everything
// written so far has been flushed.
// getclip on SAM text: a line in the middle of the text can be refused when passes before it have been written, and every piece a .gz output gets is a whole
// gzip member.  The outputs of such a command are emptied when it dies, so that none is left looking complete; appends hold the lock shared.
static std::shared_mutex g_outputs_mu;
static vector<string> g_outputs_unfinished;
static bool g_dying = false;
static vector<string> g_outputs_refused; // `run -M`: what the run created before its input turned out not to be coordinate sorted is taken away again

[[noreturn]] static void die(const string &msg)
{
	{
		std::unique_lock<std::shared_mutex> lk(g_outputs_mu);
		g_dying = true;
		for (const string &p : g_outputs_unfinished) if (truncate(p.c_str(), 0) != 0) {} // (nothing more can be done about it here)
		for (const string &p : g_outputs_refused) if (unlink(p.c_str()) != 0) {}
	}
	cerr << msg << endl;
	cout.flush(); cerr.flush(); fflush(nullptr);
	_exit(1);
}

// The end of a command: every output file is closed by now.  Handing multi-GB device buffers and page-locked staging memory back one
// hipFree / hipHostFree at a time takes 0.3-0.4 s; the process is about to end and the driver reclaims all of it at once, so the context is
// only drained (SSV_CLEAN_EXIT=1 - sanitizer and leak-check runs - destroys it the long way, and main() returns instead of _exit).
static const bool kCleanExit = getenv("SSV_CLEAN_EXIT") != nullptr;
static bool g_verify_crc = false; // -C: the device decoder checks the CRC32 of every BGZF block it inflates
static void check(ssv_ctx *ctx, int rc) { if (rc != SSV_OK) die(string("[seeksv] ") + ssv_last_error(ctx)); } // a library call that must not fail

[[noreturn]] static void usage_top()
{
	cerr << "Program: seeksv (structural variation / virus integration detection; MI355X build of the soft-clip hot path)\n"
	     << "Version: " << kVersion << "\n\n"
	     << "Usage: seeksv <command> [options]\n\n"
	     << "Command: getclip\tget soft-clipped reads\n"
	     << "         getsv  \tget final sv\n"
	     << "         somatic\tget somatic sv\n"
	     << "         realign\talign the clipped sequences of getclip to a reference (stand-in for the pipeline's external `bwa mem` step)\n"
	     << "         run    \tgetclip + realign + getsv in one process: the BAM is decoded once and stays in GPU memory" << endl;
	exit(1);
}

[[noreturn]] static void usage_getclip()
{
	cerr << "Usage: seeksv getclip [options] <input.sorted.bam>\n\n"
	     << "<input> whose name does not end in .bam is SAM text (plain or gzip; - is standard input, e.g. `samtools view -h in.cram | seeksv getclip -`):\n"
	     << "it is read once and always decoded on the GPU (-Z and -C change nothing for it), and -N above 1 is refused.  The original alignments as SAM\n"
	     << "text for `getsv` and `somatic` run as commands of their own are not supported (a pipe cannot be read twice): use `seeksv run`.\n\n"
	     << "Options: -t <double>           Threshold of match rate while combining two soft-clipped reads [0.9]\n"
	     << "         -q <int>              Minimum mapping quality of soft-clipped reads [1]\n"
	     << "         -s                    Save the low quality sequence clipped before alignment by bwa.\n"
	     << "         -o <string>           Prefix of output files [output]\n"
	     << "         -G <int>[,<int>...]   GPU ordinal(s) [0; with -N: all GPUs of the machine in order]\n"
	     << "         -N <int>              cut the BAM into N runs of records, one per GPU (ranks share GPUs when there are fewer) [1]\n"
	     << "         -H <int>              with -N: halo in bp before a run's first record (>= the longest reference span of a read) [65536]\n"
	     << "         -Z                    inflate and decode the BAM on the GPU (compressed blocks over PCIe) instead of on the host threads" << endl
	     << "         -C                    with -Z: check every BGZF block's CRC32 on the GPU (off: like libbam 0.1.16, which checks none)" << endl;
	exit(1);
}

[[noreturn]] static void usage_getsv()
{
	cerr << "Usage: seeksv getsv [options] <input clipped sequence bam or SAM text> <input orignal sorted bam> <soft-clipped reads file(*clip.gz)> <output SVs> <output unmaped clipped sequence fastq>\n"
	     << "         <input clipped sequence ...>: a name ending in .bam is BAM; every other name SAM text (plain or gzip, e.g. `bwa mem` output as it is), parsed on the GPU;\n"
	     << "                               - is standard input (SAM text)\n"
	     << "Options: -F <FILE>             Samfile/Bamfile of connected read-through reads (split alignments, e.g. bwa bwasw): their junctions are evaluated in addition;\n"
	     << "                               a name ending in .bam is BAM, every other name SAM text (plain or gzip), which is parsed on the GPU\n"
	     << "         -w <int>              Minimum mapping quality of the -F reads [1]\n"
	     << "         -B <FILE>             junction table (23 columns, as written by getsv) to evaluate in addition\n"
	     << "         -l <int>              Maximum search length to find microhomology [50]\n"
	     << "         -q <int>              Minimum mapping quality of discordant read pair [20]\n"
	     << "         -n <int>              Number of read pairs used to calculate insert size [5000000]; < 100000 switches the discordant pass off\n"
	     << "         -b <int>              Minimum number of soft clipping reads (left + right) [3]\n"
	     << "         -d <int>              Minimum distance between the two breakpoints [50]\n"
	     << "         -D                    Do not calculate depth of the breakpoints and their ajacency regions (sets -f 0)\n"
	     << "         -e <int>              Minimum number of read pairs which support the junction [0]\n"
	     << "         -f <double>           Minimum mutation frequency [0.1]\n"
	     << "         -T <int>              Maximum length of microhomology [50]\n"
	     << "         -m <int>              Minimum length of up_seq / down_seq when no read pair supports the junction [30]\n"
	     << "         -i <int>              Maximum indel number of up_seq / down_seq when no read pair supports the junction [1]\n"
	     << "         -L <int>              Flank length for the average depths [200]\n"
	     << "         -t <double> -Q <int>  accepted for compatibility\n"
	     << "         -G <int>[,<int>...]   GPU ordinal(s) [0; with -N: all GPUs of the machine in order]\n"
	     << "         -N <int>              cut the BAM into N runs of records, one per GPU; the ranks' tallies and depths meet in one RCCL all-gather [1]\n"
	     << "         -Z                    inflate and decode the BAM on the GPU (compressed blocks over PCIe) instead of on the host threads" << endl
	     << "         -C                    with -Z: check every BGZF block's CRC32 on the GPU (off: like libbam 0.1.16, which checks none)" << endl;
	exit(1);
}

[[noreturn]] static void usage_somatic()
{
	cerr << "Usage: seeksv somatic [options] <input normal original bam> <input normal soft-clipped reads file(*.clip.gz)> <input tumor SV file> <output somatic SV file>\n"
	     << "       seeksv somatic -K [-c \"getclip options\"] [options] <input normal original bam> <input tumor SV file> <output somatic SV file>\n\n"
	     << "         -K                    no clip.gz: the normal BAM is decoded once and stays in GPU memory, its soft-clip clusters are built there as `getclip` builds\n"
	     << "                               them and looked up on the GPU; the output is that of `getclip` on the normal followed by `somatic`.  Writes no other file.\n"
	     << "                               Not with -N above 1; the normal must be a BAM\n"
	     << "         -c <string>           with -K: options of the clip pass, as `getclip` takes them (-t, -q, -s; not -N, -G, -o)\n"
	     << "         -M                    with -K: mark duplicate read pairs of the normal (flag 0x400) on the GPU where its records are retained, before any pass reads a\n"
	     << "                               flag: the output of `somatic -K` on the same BAM with those flags set.  The rule and its limits: `seeksv run`'s -M\n"
	     << "         -D                    with -K: mark duplicate pairs of the normal by the unclipped 5' ends of both reads, mates joined by read name, once all its records\n"
	     << "                               are retained: the output of `somatic -K` on the same BAM with those flags set.  The rule and its limits: `seeksv run`'s -D.\n"
	     << "                               Not with -M\n"
	     << "         -L <file>             with -K: keep only the normal's records that overlap a region of this BED file, behind -M / -D and in front of every pass: the\n"
	     << "                               output of `somatic -K` on a normal that holds the kept records.  The rule and the file's form: `seeksv run`'s -L.  Not with -X\n"
	     << "         -X <file>             with -K: keep only the normal's records that overlap NO region of this BED file.  The rule: `seeksv run`'s -X.  Not with -L\n"
	     << "         -t <double>           Threshold of match rate while comparing two soft-clipped reads [0.9]\n"
	     << "         -q <int>              Minimum mapping quality of discordant read pair [20]\n"
	     << "         -l <int>              Maximum search length to find microhomology [30]\n"
	     << "         -m <int>              Minimum length of the clipped sequence  in normal [10]\n"
	     << "         -n <int>              Number of read pairs used to calculate insert size [5000000]; < 100000 switches the insert-size pass off\n"
	     << "         -G <int>[,<int>...]   GPU ordinal(s) [0; with -N: all GPUs of the machine in order]\n"
	     << "         -N <int>              cut the normal BAM into N runs of records, one per GPU; the ranks' tallies meet in one RCCL all-gather [1]\n"
	     << "         -Z                    inflate and decode the BAM on the GPU (compressed blocks over PCIe) instead of on the host threads" << endl
	     << "         -C                    with -Z: check every BGZF block's CRC32 on the GPU (off: like libbam 0.1.16, which checks none)" << endl;
	exit(1);
}

static const char CIGAR_CHARS[] = "MIDNSHP=X";

// .gz output: text is collected and written as gzip members compressed in parallel by libseeksv_host (ssvh_gz_append)
struct GzOut {
	string path, buf;
	bool started = false;
	bool open(const string &p)
	{
		path = p;
		FILE *f = fopen(p.c_str(), "wb"); // like ogzstream: fail early when the file cannot be created
		if (!f) return false;
		fclose(f);
		return true;
	}
	void flush(bool final)
	{
		if (buf.empty() && (started || !final)) return;
		int rc;
		{
			std::shared_lock<std::shared_mutex> lk(g_outputs_mu);
			if (g_dying) return;
			rc = ssvh_gz_append(path.c_str(), buf.data(), buf.size(), started ? 1 : 0);
		}
		if (rc != 0) die(string("[seeksv] ") + ssvh_last_error());
		started = true;
		buf.clear();
	}
	void write(const string &s) { buf += s; if (buf.size() >= ((size_t)256 << 20)) flush(false); }
	void write_parts(const vector<string> &parts) // large, already formatted pieces: compressed from where they lie
	{
		flush(false);
		vector<const char *> ptr; vector<size_t> len;
		for (auto &s : parts) if (!s.empty()) { ptr.push_back(s.data()); len.push_back(s.size()); }
		if (ptr.empty()) return;
		int rc;
		{
			std::shared_lock<std::shared_mutex> lk(g_outputs_mu);
			if (g_dying) return;
			rc = ssvh_gz_append_v(path.c_str(), ptr.data(), len.data(), (int)ptr.size(), started ? 1 : 0);
		}
		if (rc != 0) die(string("[seeksv] ") + ssvh_last_error());
		started = true;
	}
	void close() { flush(true); }
};

// ---------------------------------------------------------------------------------------------------------------------
// where the record batches come from: the host reader (inflate + decode on the host threads, batches uploaded by the kernels' H2D
// staging), or -Z: the compressed BGZF blocks go to the GPU as they are and are inflated and decoded there (ssv_bamdec_*); a reader
// thread fills one pinned staging buffer while the chunk in the other one is being decoded.
// ---------------------------------------------------------------------------------------------------------------------

// Page-locked batch arrays for the host reader (copies to the GPU out of them run asynchronously).
static void *pinned_alloc(size_t n) { void *p = nullptr; return ssv_host_alloc(n, &p) == SSV_OK ? p : nullptr; }
static void pinned_release(void *p) { ssv_host_free(p); }
static void use_pinned_batches(ssvh_bam *b)
{
	ssvh_bam_set_allocator(b, pinned_alloc, pinned_release);
	ssvh_bam_set_readahead(b, 1);
}

// The batches of a host reader (read-ahead on: three sets of arrays) through a context: batch k+1 is decoded, announced and on its way to the
// GPU (ssv_batch_prefetch, the upload stream) while batch k is scanned; `side` sees every batch right after it was read (the reader's
// per-batch side channel - unmapped reads - is valid only then), `scan` gets them in order.  Returns "" or the error text.
// records per batch of the host reader (SSV_HOST_BATCH_RECORDS: tests cut small files into many batches)
static int64_t host_batch_records()
{
	static const int64_t n = [] { const char *e = getenv("SSV_HOST_BATCH_RECORDS"); return e ? std::max<int64_t>(1, atoll(e)) : (int64_t)1 << 22; }();
	return n;
}

template <class Side, class Scan> static string pump_host_batches(ssvh_bam *rb, ssv_ctx *ctx, int keep_all_seq, Side side, Scan scan)
{
	ssv_batch_t b[2];
	auto read = [&](ssv_batch_t *out) -> string {
		if (ssvh_bam_read_batch(rb, host_batch_records(), keep_all_seq, out) != 0) return string("[seeksv] ") + ssvh_last_error();
		if (out->n == 0) return "";
		side(*out);
		if (ssv_batch_prefetch(ctx, out) != SSV_OK) return string("[seeksv] ") + ssv_last_error(ctx);
		return "";
	};
	string err = read(&b[0]);
	for (int k = 0; err.empty() && b[k & 1].n != 0; ++k) {
		err = read(&b[(k + 1) & 1]);
		if (!err.empty()) break;
		err = scan(b[k & 1]);
	}
	return err;
}

// `seeksv run`: one process, one context, one decode of the BAM.  While getclip scans the file, every decoded batch is copied into device
// memory of its own (ssv_batch_retain: hot columns, one 64-byte line per record, CIGARs, bases of the soft-clipped reads: 80 B/record -
// a 30x genome is 50 GB of the GPU's 288); the getsv passes of the same process then find the file's records there instead of reading,
// inflating and decoding the file a second and third time (the reference does: cluster.cpp:48, getsv.cpp:1067, bam2depth.h:29).
//
// `seeksv run -N n`: what the ranks' getclip leaves behind for the getsv pass of the same process - per rank its context (alive after rank_main) and the
// batches of its OWN run, copied into that context's memory (ssv_batch_retain, 80 B a record; the halo is scanned and forgotten), and the cuts of the file
// both steps share.  A batch is only ever scanned by the context that holds it.
struct RunRank {
	ssv_ctx *ctx = nullptr;      // (rank 0: the context acquire_ctx hands to the later steps of the process)
	int device = 0;
	vector<ssv_batch_t> batches; // in file order
	int64_t kept = 0;            // records in them
};
struct RunRanks {
	vector<ssvh_bam_part> parts;
	vector<RunRank> rank;        // (empty: a run without -N)
	bool fell_back = false;      // contigs that come back: the ranks gave way to getclip_single, nothing of theirs is left
	void release() // every batch, and every context but rank 0's (the process's own)
	{
		for (size_t r = 0; r < rank.size(); ++r) {
			RunRank &k = rank[r];
			if (k.ctx) for (auto &b : k.batches) ssv_batch_release(k.ctx, &b);
			k.batches.clear(); k.kept = 0;
			if (r > 0 && k.ctx) { ssv_ctx_destroy(k.ctx); k.ctx = nullptr; }
		}
	}
};

// `seeksv run`: the reference is read (and packed to 2 bits) by a thread of its own while getclip runs
struct PrereadFasta {
	std::thread th;
	bool ok = false;
	vector<string> names; vector<int32_t> lens; vector<int64_t> offs = vector<int64_t>(1, 0); vector<uint64_t> words;
};

// What the steps of one `seeksv run` hand to each other.  cmd_run owns the one session of the process (on the heap, never destroyed: die() may exit while
// the ranks', the aligner's or the reference reader's threads run) and passes a pointer to the step bodies with the call that works on the run's own BAM;
// stand-alone commands - and sources opened for any other file - pass nullptr.
struct RunSession {
	ssv_ctx *ctx = nullptr;      // the context every step of the run shares
	bool collect = false;        // getclip_single keeps what it decodes (batches) and what it formats (pieces)
	vector<ssv_batch_t> batches; // in file order
	bool rows_kept = false;      // the pieces below are prefix.clip.gz / prefix.clip.fq.gz (the files are written all the same: they are outputs)
	// their decompressed contents, in the pieces the formatting threads made (whole rows / whole records each; never glued together: appending 2.5 GB to
	// one string on one thread was a second of `seeksv run`) - and, since round 6, what the formatter knew while it wrote them: every row as views into
	// its text (the junction stage parsed 5.5 M rows back out of it: 0.35 s) and where every FASTQ record's sequence and qualities lie (the aligner
	// step cut the text into lines again: 0.2 s).  `clean`: every row is what the text parser would make of it (nine non-empty fields, no white space).
	struct FqRef { uint32_t seq_off, seq_len, qual_off, qual_len; };
	struct Piece { string rows, fq; vector<seeksv::ClipRow> parsed; vector<FqRef> reads; bool clean = true; };
	std::deque<Piece> pieces;    // (a deque: a piece never moves, the views stay good)
	std::function<void(const vector<Piece *> &)> on_pass; // called by getclip's output thread with the pieces of the pass it has just written
	// `seeksv somatic -K`: the pass exists for its records (kept, as above) and for the look-ups the library runs against every pass's table (ssv_clip_probe_set):
	// no output file is opened, no row is formatted, the unmapped pairs are not collected, and getclip's own stderr lines are not printed
	bool probe_only = false;
	bool all_clean() const { for (const Piece &p : pieces) if (!p.clean) return false; return true; }
	vector<seeksv::TextView> row_views() const { vector<seeksv::TextView> v; for (const Piece &p : pieces) v.push_back(seeksv::TextView{p.rows.data(), p.rows.size()}); return v; }
	// what the aligner step made of the clipped sequences (clip.bam is written all the same); the read names point into the pieces' FASTQ text
	struct Aligned { const struct AlignedRecords *rec = nullptr; vector<string> names; } aln; // (the run's aligner thread owns the records)
	std::thread bam_writer;      // clip.bam of `seeksv run`, written beside getsv
	// `seeksv run -P`: the text of prefix.unmapped_1.fq / _2.fq as the side channel's sinks wrote it, piece by piece in file order (whole records each)
	bool keep_unmapped = false;
	std::deque<string> unmapped[2];
	std::function<void(ssv_ctx *, int, JunctionMap &)> split_leg; // ... and the -F pass without a file over them (run_split_leg), called where getsv runs its -F pass
	// `seeksv run -A`: getclip's pump sent every decoded chunk through the split-read session of `ctx` (ssv_rt_begin_original); getsv finishes it where it
	// runs its -F pass.  The contigs' names, and with SSV_TIMING what the scans took (the groups are reset by later stages)
	bool splitread_open = false, splitread_sa = false;
	double splitread_aux_ms = 0; int64_t splitread_aux_launches = 0;
	vector<string> splitread_names;
	double splitread_scan_ms = 0; int64_t splitread_scan_launches = 0; double splitread_scan_wall = 0;
	// `seeksv run -N n`: the ranks of getclip keep their own runs; rank 0's context is `ctx`.  Nothing above is collected until a file whose contigs come
	// back sends the run down the one-GPU path.
	RunRanks ranks;
	bool ranked() const { return !ranks.rank.empty() && !ranks.fell_back; }
	void fall_back() { ranks.release(); ranks.fell_back = true; collect = true; } // from here on the run is `seeksv run` on the first device: one context, which keeps every record
	PrereadFasta preread;        // the reference, handed to the aligner step that reads it
	// the run's input is SAM text (a name without ".bam": plain, gzip or "-"), which can be read once: its @SQ list, kept by getclip for the getsv step's header
	bool text_input = false;
	vector<string> text_names; vector<int32_t> text_lens;
};

static void release_ctx(ssv_ctx *ctx, const RunSession *run)
{
	if (run && ctx == run->ctx) return; // shared by the steps of `seeksv run`, which lets go of it at its end
	if (kCleanExit) ssv_ctx_destroy(ctx);
	else ssv_sync(ctx);
}

// The HIP runtime takes 0.1-0.3 s to come up (first call of the process) - longer than a command spends on a 6 GB file's kernels.  main() starts the
// context on a thread of its own before the command parses its arguments; opening files, the junction stage of getsv and the reader's first chunks
// run beside it, and acquire_ctx joins it where the first kernel is needed.
struct EarlyCtx {
	std::thread th;
	ssv_ctx *ctx = nullptr;
	int device = -1, rc = SSV_OK;
	string err;
	bool started = false, taken = false;
};
static EarlyCtx g_early;
static void early_ctx_join() { if (g_early.th.joinable()) g_early.th.join(); }
static void early_ctx_start(int device)
{
	if (g_early.started) return;
	g_early.started = true; g_early.device = device;
	atexit(early_ctx_join); // (usage errors leave through exit(): not while a thread is inside the runtime's start-up)
	g_early.th = std::thread([] {
		g_early.rc = ssv_ctx_create(g_early.device, &g_early.ctx);
		if (g_early.rc != SSV_OK) g_early.err = ssv_last_error(nullptr);
	});
}

static ssv_ctx *acquire_ctx(int device, const RunSession *run)
{
	if (run && run->ctx) return run->ctx;
	if (g_early.started && !g_early.taken) {
		early_ctx_join();
		g_early.taken = true;
		if (g_early.device == device) {
			if (g_early.rc != SSV_OK) die(string("[seeksv] ") + g_early.err);
			return g_early.ctx;
		}
		if (g_early.ctx) ssv_ctx_destroy(g_early.ctx); // (another -G than the one main() saw)
	}
	ssv_ctx *ctx = nullptr;
	if (ssv_ctx_create(device, &ctx) != SSV_OK) die(string("[seeksv] ") + ssv_last_error(nullptr));
	return ctx;
}

static const bool kTimingChunks = [] { const char *e = getenv("SSV_TIMING"); return e ? atoi(e) : 0; }() >= 2; // SSV_TIMING=2: per-chunk detail

// Staging memory for the chunks of a file in copy mode.  hipHostMalloc hands out page-locked memory at 0.25 s/GB (it allocates, clears and locks on
// one thread, and other HIP calls of the process queue behind it meanwhile): three 0.6-1.5 GB buffers were 0.5 s before the first kernel of a
// command.  Here a buffer is plain anonymous memory; the reader threads' pread calls fault its pages in on all cores while they fill it for the
// first time, and only then are the pages that hold bytes page-locked (ssv_host_register: 0.03 s/GB).  Buffers go back to a process-wide pool when a
// source closes (`seeksv run`, the ranks' halo and own passes: the next source finds them locked already).
struct StageBuf {
	uint8_t *p = nullptr;
	size_t cap = 0, locked = 0; // locked: bytes from p on that are page-locked
	void *map_base = nullptr; size_t map_len = 0; // the mapping p lies in (p is 2 MB aligned)
	int near_device = 0;                          // the GPU its pages should lie beside
	static size_t page() { static const size_t v = (size_t)sysconf(_SC_PAGESIZE); return v; }
	bool reserve(size_t want)
	{
		if (cap >= want) return true;
		release();
		// on transparent huge pages where the kernel grants them (2 MB aligned, madvise): 512 times fewer pages to fault in, to lock and - when the process ends -
		// to unlock (tools/exit_cost.cpp: 4 GB of locked 4 KB pages cost 0.4 s between _exit and the caller's wait() returning, huge pages 0.001 s)
		const size_t huge = (size_t)2 << 20;
		const size_t n = (want + huge - 1) & ~(huge - 1);
		void *m = mmap(nullptr, n + huge, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
		if (m == MAP_FAILED) return false;
		map_base = m; map_len = n + huge;
		p = reinterpret_cast<uint8_t *>(((uintptr_t)m + huge - 1) & ~(uintptr_t)(huge - 1)); cap = n;
		(void)madvise(p, n, MADV_HUGEPAGE);
		ssv_host_bind_near(p, n, near_device); // (the reader's pread threads run on any CPU: the pages still land beside the GPU that fetches them)
		return true;
	}
	// the first `filled` bytes have just been written: make sure they are page-locked (a buffer that is mostly full is locked whole, its tail
	// touched on a few threads first, so that chunks of slightly different sizes do not lock again and again)
	bool lock(size_t filled)
	{
		if (filled <= locked) return true;
		if (locked) { ssv_host_unregister(p); locked = 0; }
		size_t n = (filled + page() - 1) & ~(page() - 1);
		if (filled * 2 > cap) {
			const int nt = 8;
			vector<std::thread> th;
			for (int t = 0; t < nt; ++t) th.emplace_back([&, t] {
				const size_t lo = n + (cap - n) / page() * (size_t)t / nt * page(), hi = n + (cap - n) / page() * (size_t)(t + 1) / nt * page();
				for (size_t o = lo; o < hi; o += page()) p[o] = 0;
			});
			for (auto &x : th) x.join();
			n = cap;
		}
		if (ssv_host_register(p, n) != SSV_OK) return false; // (the copies out of it then go through the runtime's own staging: slower, still right)
		locked = n;
		return true;
	}
	void release()
	{
		if (!p) return;
		if (locked) ssv_host_unregister(p);
		munmap(map_base, map_len);
		p = nullptr; cap = locked = 0; map_base = nullptr; map_len = 0;
	}
};
static int g_near_device = 0; // the command's GPU (-G; main() sets it): where page-locked staging memory should lie
static std::mutex g_stage_pool_mu;
static vector<StageBuf> g_stage_pool;
static StageBuf stage_from_pool(size_t want)
{
	std::lock_guard<std::mutex> lk(g_stage_pool_mu);
	for (size_t k = 0; k < g_stage_pool.size(); ++k)
		if (g_stage_pool[k].cap >= want) { StageBuf b = g_stage_pool[k]; g_stage_pool.erase(g_stage_pool.begin() + (long)k); return b; }
	return StageBuf();
}
static void stage_to_pool(StageBuf &b)
{
	if (!b.p) return;
	std::lock_guard<std::mutex> lk(g_stage_pool_mu);
	if (g_stage_pool.size() < 8) g_stage_pool.push_back(b); else b.release();
	b = StageBuf();
}

static bool is_bam_name(const string &path) { return path.size() >= 4 && path.rfind(".bam") == path.size() - 4; }

static void *sam_stage_alloc(size_t bytes) { void *p = nullptr; return ssv_host_alloc(bytes, &p) == SSV_OK ? p : nullptr; }
static void sam_stage_free(void *p) { ssv_host_free(p); }

// A SAM text file through the device decoder: the header on the host, the records' text to the GPU as it is, in chunks cut anywhere (SSV_SAM_CHUNK_KB: their
// size, 256 MB by default); a reader thread fills page-locked buffers ahead, and chunk k + 1 crosses the host link under chunk k's kernels
// (ssv_samdec_prefetch).  open(): the header, with libbam's [samopen] line; begin(): the decoder and the reader thread - sorted: a coordinate-sorted original
// (ssv_samdec_sorted: batches as the BAM decoder gives them, and the chunk's lists); next(): the next chunk's batch and names, valid until the call after.
// The one loop behind the -F pass, the pass over the clipped-sequence re-alignments (sam_text_pass) and the original alignments of getclip and run (BatchSource).
struct SamTextDecoder {
	seeksv::SamTextReader rd;
	ssv_ctx *ctx = nullptr;
	bool ended = false, over = false, sorted = false;
	bool keep_all_seq = false; // (run -D: every record's bases + qualities, set before begin())
	ssv_names_t names{};
	void open(const string &path, const char *open_error)
	{
		string err;
		if (!rd.open(path, err)) die(open_error);
		if (rd.target_names().empty()) { // (the reference goes on and aborts at its first record: "[sam_read1] missing header? Abort!")
			cerr << "[samopen] no @SQ lines in the header." << endl;
			die(open_error);
		}
		cerr << "[samopen] SAM header is present: " << rd.target_names().size() << " sequences." << endl;
	}
	void begin(ssv_ctx *c, bool sorted_original)
	{
		ctx = c; sorted = sorted_original;
		vector<const char *> cnames;
		for (const string &s : rd.target_names()) cnames.push_back(s.c_str());
		ssv_samdec_params sp;
		memset(&sp, 0, sizeof(sp));
		sp.n_targets = (int32_t)cnames.size(); sp.target_names = cnames.data(); sp.first_line = rd.first_record_line();
		check(ctx, ssv_samdec_begin(ctx, &sp));
		if (sorted) check(ctx, ssv_samdec_sorted(ctx, keep_all_seq ? 1 : 0));
		const char *e = getenv("SSV_SAM_CHUNK_KB");
		const size_t chunk = e && atoll(e) > 0 ? (size_t)atoll(e) << 10 : (size_t)256 << 20;
		rd.start(chunk, sam_stage_alloc, sam_stage_free);
	}
	void decode(const void *text, size_t bytes, int last, ssv_batch_t *b)
	{
		if (ssv_samdec_decode(ctx, text, bytes, SSV_MEM_HOST, last, b) != SSV_OK) {
			const string m = ssv_last_error(ctx);
			die(m.compare(0, 11, "Parse error") == 0 ? m : "[seeksv] " + m);
		}
		check(ctx, ssv_samdec_names(ctx, &names));
	}
	// false: the file is over (every chunk has been decoded)
	bool next(ssv_batch_t *b)
	{
		if (over) return false;
		seeksv::SamTextReader::Chunk ck, nx;
		string err;
		if (rd.next(ck, err)) {
			if (!ck.last && rd.ready_behind(nx)) check(ctx, ssv_samdec_prefetch(ctx, nx.data, nx.bytes));
			decode(ck.data, ck.bytes, ck.last ? 1 : 0, b);
			ended = ck.last;
			return true;
		}
		if (!err.empty()) die(err);
		over = true;
		if (ended) return false;
		decode(nullptr, 0, 1, b);
		ended = true;
		return true;
	}
	void close()
	{
		if (ctx) check(ctx, ssv_sync(ctx)); // (the staging buffers go with the reader)
		rd.close();
	}
};

// The one place a text input's contigs come from: the @SQ SN: / LN: list of its header behind the handle every step asks for names and lengths
// (ssvh_bam_target_name, ssvh_bam_target_lens, ssvh_plan_create) - a handle with no file behind it
static ssvh_bam *text_header_handle(const vector<string> &names, const vector<int32_t> &lens)
{
	vector<const char *> z;
	for (const string &n : names) z.push_back(n.c_str());
	ssvh_bam *h = nullptr;
	if (ssvh_bam_from_header(z.data(), lens.data(), (int32_t)z.size(), &h) != 0) die(string("[seeksv] ") + ssvh_last_error());
	return h;
}

struct BatchSource {
	ssvh_bam *bam = nullptr;
	ssv_ctx *ctx = nullptr;
	bool on_device = false;
	const RunSession *resident = nullptr; // the records are in HBM already: the run's retained batches
	bool any_order = false;    // a file in any record order (getsv -F: split alignments in read order; run -u) - ssv_bamdec_any_order, ssv_samdec_any_order
	size_t resident_next = 0;
	// ---- device mode: a reader thread runs up to three chunks ahead of the decoder ----
	// A chunk = whole BGZF blocks, the file's bytes as they are.  Two ways to get them to the GPU:
	//   copy (default): all host threads pread the chunk into one of three staging buffers (StageBuf above: locked after their first fill);
	//   map  (SSV_READER=map): the file is mapped and the chunk's pages are page-locked where they lie in the page cache (ssv_host_register), the GPU's
	//         DMA engines fetch them there and no CPU copies the file.  Measured on a 11.8 GB file (profiles/r04_cli_reader_modes.txt): locking a fresh
	//         mapping's pages costs 0.04-0.1 s/GB on the one thread the driver lets do it (page-table entries for every 4 KB page first), i.e. 25-60 ms
	//         per 0.6 GB chunk where the copy takes 14 ms on 16 threads, and unmapping the file at the end 0.19 s: slower, kept for boxes with few CPUs.
	// Either way chunk k+1 is announced to the upload stream (ssv_bamdec_prefetch) before chunk k is decoded, so its bytes cross PCIe under chunk k's
	// kernels, while the reader prepares chunk k+2.
	static constexpr int NS = 3;
	struct Slot {
		StageBuf stage;                                       // copy mode: the slot's staging buffer
		void *reg_base = nullptr; size_t reg_bytes = 0;       // map mode: the page range that is locked for this slot's chunk
		const uint8_t *data = nullptr; size_t n_bytes = 0;    // the chunk
		vector<ssv_bgzf_block> blocks; int64_t n_blocks = 0;
		uint64_t limit = UINT64_MAX;                          // ssvh_bam_raw_limit: where a range of records ends inside the chunk
		bool last = false;                                    // nothing but the end-of-file block can follow
		double t_fill = 0;
		string err;
	} slot[NS];
	size_t stage_bytes = 0, first_bytes = 0;
	uint64_t chunk_inflated = 0;
	bool map_mode = true;
	std::thread reader;
	std::mutex mu;
	std::condition_variable cv;
	int64_t produced = 0, released = 0, cur = 0; // chunks the reader has finished / the decoder has let go of / next chunk to decode
	bool reader_exit = false, stop_reader = false;
	int64_t announced = -1;                      // highest chunk handed to ssv_bamdec_prefetch
	bool at_end = false, end_pending = false;
	uint64_t file_bytes = 0;
	ssv_bamdec_info info{};
	// ---- SAM text (a name without ".bam"): always decoded on the GPU, in the decoder's mode for coordinate-sorted originals - `info` is ssv_samdec_lists' ----
	SamTextDecoder *text = nullptr;
	// the header of a text input before anything is created (the reference's samopen: its [samopen] line, a missing file, a header without @SQ); open() goes on from it
	void open_text_header(const string &path, const char *open_error)
	{
		text = new SamTextDecoder;
		text->open(path, open_error);
		bam = text_header_handle(text->rd.target_names(), text->rd.target_lens());
	}

	// a run of records [start, end) of the file instead of all of it (virtual offsets of ssvh_bam_partition); before open()
	bool ranged = false;
	uint64_t r_start_coff = 0, r_end_coff = 0;
	uint32_t r_start_uoff = 0, r_end_uoff = 0;
	void set_range(uint64_t sc, uint32_t su, uint64_t ec, uint32_t eu) { ranged = true; r_start_coff = sc; r_start_uoff = su; r_end_coff = ec; r_end_uoff = eu; }
	int32_t r_prev_tid = 0; // contig of the last mapped-pair record before the range

	void open(const string &path, ssv_ctx *c, bool device_inflate, const char *open_error) { open(path, [c] { return c; }, device_inflate, open_error); }
	// get_ctx: asked for the context as late as possible - the file is opened and the reader thread is on its first chunks before (the context of a
	// fresh process may still be coming up, acquire_ctx).  run: `seeksv run` opening its own BAM - whole, and once getclip has kept its batches in this
	// context, they are the source (every other file, -F's among them, is opened without: the caller knows which file is which)
	void open(const string &path, const std::function<ssv_ctx *()> &get_ctx, bool device_inflate, const char *open_error, const RunSession *run = nullptr)
	{
		on_device = device_inflate;
		if (!is_bam_name(path)) {
			on_device = true;
			if (ranged) die("[seeksv] SAM text is read from its start to its end: runs of records (-N) need a BAM");
			if (run && !run->collect) { // a step behind the run's getclip: the records are in HBM, the text is gone
				ctx = get_ctx();
				if (!run->text_input || run->ctx != ctx || run->batches.empty()) die("[seeksv] the original alignments as SAM text are read once, by `seeksv run`; this step would read them again");
				bam = text_header_handle(run->text_names, run->text_lens);
				resident = run;
				return;
			}
			if (!text) open_text_header(path, open_error);
			ctx = get_ctx();
			text->begin(ctx, true);
			if (any_order) check(ctx, ssv_samdec_any_order(ctx, 1));
			return;
		}
		if (ssvh_bam_open(path.c_str(), &bam) != 0) die(open_error);
		if (run || !on_device) ctx = get_ctx();
		if (run && !ranged && !run->collect && ctx && run->ctx == ctx && !run->batches.empty()) { resident = run; on_device = true; return; }
		if (!on_device) {
			if (ranged && ssvh_bam_set_range(bam, r_start_coff, r_start_uoff, r_end_coff, r_end_uoff) != 0) die(string("[seeksv] ") + ssvh_last_error());
			use_pinned_batches(bam);
			return;
		}
		const char *e1 = getenv("SSV_CHUNK_INFLATED_MB"), *e2 = getenv("SSV_STAGE_MB"), *e4 = getenv("SSV_READER");
		map_mode = e4 && !strcmp(e4, "map");
		{
			FILE *f = fopen(path.c_str(), "rb");
			if (f) { fseek(f, 0, SEEK_END); file_bytes = (uint64_t)ftell(f); fclose(f); }
			// What a command pays once grows with the chunk size: ~3.8 bytes of device memory per inflated byte and three page-locked staging buffers, to set
			// up AND to give back (the kernel takes 0.16-0.25 s to tear a process with 8 GB of device buffers and 2.3 GB of locked pages down, after exit and
			// before the caller's wait returns).  Since round 4 both inflate passes are a wavefront per block and their rate does not depend on the blocks in
			// flight: chunks of 1 GB inflated (0.3 GB of file) whatever the file's size (round 3: up to 4 GB, which the lane-per-block kernels needed; until late in
			// round 4 2 GB above 16 GB of file - measured again on the 23.7 GB and 47.4 GB files: 1 GB chunks take 9-11 % off both commands, half of it after exit).
			chunk_inflated = (uint64_t)(e1 ? atoll(e1) : 1024) << 20;
			stage_bytes = (size_t)(e2 ? atoll(e2) : 384) << 20;
			if (file_bytes && file_bytes + 65536 < stage_bytes) stage_bytes = (size_t)file_bytes + 65536;
		}
		uint64_t first = 0;
		if (ranged) { if (ssvh_bam_raw_begin_range(bam, r_start_coff, r_start_uoff, r_end_coff, r_end_uoff, &first) != 0) die(string("[seeksv] ") + ssvh_last_error()); file_bytes = 0; }
		else if (ssvh_bam_raw_begin(bam, &first) != 0) die(string("[seeksv] ") + ssvh_last_error());
		// The file's first chunk is the one nothing overlaps with: a small one (128 MB: read and locked in ~10 ms), so that the GPU starts early
		first_bytes = std::min(stage_bytes, first_bytes_default());
		reader = std::thread([this] { reader_main(); }); // (reads, and locks its buffers: needs no context)
		if (!ctx) ctx = get_ctx();
		check(ctx, ssv_bamdec_begin(ctx, ssvh_bam_n_targets(bam), first));
		check(ctx, ssv_bamdec_target_lens(ctx, ssvh_bam_target_lens(bam)));
		if (g_verify_crc) ssv_bamdec_verify_crc(ctx, 1);
		if (any_order) check(ctx, ssv_bamdec_any_order(ctx, 1));
		if (ranged) ssv_bamdec_prev_tid(ctx, r_prev_tid);
		if (!file_bytes || file_bytes > first_bytes_default()) ssv_bamdec_expect(ctx, chunk_inflated);
	}
	static size_t page_size() { static const size_t p = (size_t)sysconf(_SC_PAGESIZE); return p; }
	static size_t first_bytes_default() { return (size_t)128 << 20; }
	int near_device = g_near_device; // the GPU that fetches this source's chunks: their staging pages are asked for on its NUMA node
	bool take_stage(Slot &S, size_t want)
	{
		if (S.stage.cap >= want) return true;
		stage_to_pool(S.stage);
		S.stage = stage_from_pool(want);
		S.stage.near_device = near_device;
		return S.stage.reserve(want);
	}
	// the reader thread: chunk k into slot k % NS as soon as the decoder has let go of chunk k - NS
	void reader_main()
	{
		(void)pthread_setname_np(pthread_self(), "ssv-chunks");
		for (int64_t k = 0;; ++k) {
			{
				std::unique_lock<std::mutex> lk(mu);
				cv.wait(lk, [&] { return stop_reader || k - released < NS; });
				if (stop_reader) break;
			}
			Slot &S = slot[k % NS];
			const auto t0 = std::chrono::steady_clock::now();
			if (S.reg_base) { ssv_host_unregister(S.reg_base); S.reg_base = nullptr; } // (the chunk that was here has been decoded)
			S.err.clear(); S.n_blocks = 0; S.n_bytes = 0; S.data = nullptr; S.limit = UINT64_MAX; S.last = false;
			const size_t want = k == 0 ? first_bytes : stage_bytes;
			if (S.blocks.empty()) S.blocks.resize((size_t)(std::min<uint64_t>(chunk_inflated, file_bytes ? file_bytes * 64 : chunk_inflated) >> 12) + 1024); // blocks are <= 64 KB but may be much smaller
			bool filled = false;
			if (map_mode) {
				const void *ptr = nullptr;
				const int rc = ssvh_bam_map_blocks(bam, want, chunk_inflated, S.blocks.data(), (int64_t)S.blocks.size(), &S.n_blocks, &ptr, &S.n_bytes);
				if (rc == -2) map_mode = false; // the file cannot be mapped: staging buffers from here on (nothing has been consumed)
				else if (rc != 0) S.err = ssvh_last_error();
				else {
					filled = true;
					S.data = static_cast<const uint8_t *>(ptr);
					if (S.n_bytes) {
						const uintptr_t lo = reinterpret_cast<uintptr_t>(ptr) & ~(uintptr_t)(page_size() - 1);
						const uintptr_t hi = (reinterpret_cast<uintptr_t>(ptr) + S.n_bytes + page_size() - 1) & ~(uintptr_t)(page_size() - 1);
						if (ssv_host_register(reinterpret_cast<void *>(lo), (size_t)(hi - lo)) == SSV_OK) { S.reg_base = reinterpret_cast<void *>(lo); S.reg_bytes = (size_t)(hi - lo); }
						else {
							// the runtime will not lock these pages (a file system it cannot pin, a memory-lock limit): this chunk is copied out of the
							// mapping, the following ones are read the other way
							map_mode = false;
							if (!take_stage(S, std::max(S.n_bytes + 64, stage_bytes))) S.err = "out of memory (staging buffer)";
							else { memcpy(S.stage.p, ptr, S.n_bytes); S.stage.lock(S.n_bytes); S.data = S.stage.p; }
						}
					}
				}
			}
			if (!filled && S.err.empty()) {
				// (the chunk that was in this buffer has been decoded: its bytes are on the device)
				if (!take_stage(S, stage_bytes)) S.err = "out of memory (staging buffer)";
				if (S.err.empty() && ssvh_bam_read_blocks(bam, S.stage.p, std::min(S.stage.cap, want), chunk_inflated, S.blocks.data(), (int64_t)S.blocks.size(), &S.n_blocks, &S.n_bytes) != 0) S.err = ssvh_last_error();
				if (S.err.empty() && S.n_bytes) S.stage.lock(S.n_bytes);
				S.data = S.stage.p;
			}
			if (S.err.empty()) ssvh_bam_raw_limit(bam, &S.limit);
			consumed_bytes += S.n_bytes;
			// (the chunk holds the file's bytes as they are, block headers and trailers included) when nothing but the 28-byte end-of-file block can be
			// left, no further chunk is read
			S.last = S.n_blocks == 0 || (file_bytes && consumed_bytes + 28 >= file_bytes);
			S.t_fill = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
			const bool done = S.last || !S.err.empty();
			{
				std::lock_guard<std::mutex> lk(mu);
				produced = k + 1;
				if (done) reader_exit = true;
			}
			cv.notify_all();
			if (done) break;
		}
	}
	uint64_t consumed_bytes = 0; // (reader thread)
	// the next batch (valid until the following call); false at the end of the file
	bool next(ssv_batch_t *b, int keep_all_seq)
	{
		if (resident) {
			if (resident_next >= resident->batches.size()) return false;
			*b = resident->batches[resident_next++];
			return true;
		}
		if (!on_device) {
			if (ssvh_bam_read_batch(bam, host_batch_records(), keep_all_seq, b) != 0) die(string("[seeksv] ") + ssvh_last_error());
			return b->n != 0;
		}
		if (text) {
			while (text->next(b)) {
				check(ctx, ssv_samdec_lists(ctx, &info));
				if (b->n) return true; // (a chunk can hold only the middle of one long line)
			}
			return false;
		}
		for (;;) {
			if (at_end) return false;
			if (end_pending) { // the last chunk has been handed out: tell the decoder the input is over (an unfinished record is an error)
				ssv_batch_t none;
				check(ctx, ssv_bamdec_decode(ctx, nullptr, 0, nullptr, 0, keep_all_seq, &none));
				at_end = true;
				return false;
			}
			const auto tw0 = std::chrono::steady_clock::now();
			bool next_ready = false;
			{
				std::unique_lock<std::mutex> lk(mu);
				cv.wait(lk, [&] { return produced > cur; });
				next_ready = produced > cur + 1;
			}
			const auto tw1 = std::chrono::steady_clock::now();
			Slot &S = slot[cur % NS];
			if (!S.err.empty()) die("[seeksv] " + S.err);
			const bool last_chunk = S.last;
			// the chunk behind this one starts its way over PCIe now, under this chunk's kernels
			if (!last_chunk && next_ready && announced < cur + 1) {
				Slot &N = slot[(cur + 1) % NS];
				if (N.err.empty() && N.n_blocks > 0) check(ctx, ssv_bamdec_prefetch(ctx, N.data, N.n_bytes));
				announced = cur + 1;
			}
			if (S.limit != UINT64_MAX) ssv_bamdec_limit(ctx, S.limit);
			check(ctx, ssv_bamdec_decode(ctx, S.data, S.n_bytes, S.blocks.data(), S.n_blocks, keep_all_seq, b));
			if (kTimingChunks) cerr << "[timing] (chunk of " << S.n_bytes << " bytes, " << S.n_blocks << " blocks, " << (S.reg_base ? "page-locked in the mapping" : "copied to staging") << " in " << S.t_fill
			                        << " s: waited " << std::chrono::duration<double>(tw1 - tw0).count() << " s for the reader, " << (announced >= cur && cur > 0 ? "announced ahead, " : "") << "decoded in "
			                        << std::chrono::duration<double>(std::chrono::steady_clock::now() - tw1).count() << " s)" << endl;
			const int64_t nb = S.n_blocks;
			{
				std::lock_guard<std::mutex> lk(mu);
				released = ++cur; // the chunk's bytes are on the device and decoded: its slot is the reader's again
			}
			cv.notify_all();
			if (nb == 0) { at_end = true; return false; }
			if (last_chunk) end_pending = true;
			ssv_bamdec_last(ctx, &info);
			if (b->n) return true; // (a chunk can hold only the middle of one huge record)
		}
	}
	// every batch through side(b) (right after it was read) and scan(b); with the host reader the copy of the next batch runs ahead
	template <class Side, class Scan> void pump(int keep_all_seq, Side side, Scan scan)
	{
		if (!on_device) {
			const string err = pump_host_batches(bam, ctx, keep_all_seq, side, [&](const ssv_batch_t &b) { scan(b); return string(); });
			if (!err.empty()) die(err);
			return;
		}
		ssv_batch_t b;
		while (next(&b, keep_all_seq)) { side(b); scan(b); }
	}
	// UNMAP|MUNMAP records of the current batch as they lie in the BAM stream (block_size prefixed), in order; valid while the NEXT batch is read
	void unmapped_raw(const uint8_t **raw, size_t *bytes)
	{
		if (!on_device) { ssvh_bam_unmapped_raw(bam, raw, bytes); return; }
		*raw = info.unmapped_raw; *bytes = (size_t)info.unmapped_bytes;
	}
	// ... one by one, decoded
	template <class F> void for_each_unmapped(F fn)
	{
		const char *qname, *seq, *qual; int is_read1;
		if (!on_device) {
			for (int64_t k = 0, nu = ssvh_bam_unmapped_count(bam); k < nu; ++k) { ssvh_bam_unmapped_get(bam, k, &qname, &seq, &qual, &is_read1); fn(qname, seq, qual, is_read1); }
			return;
		}
		for (size_t off = 0, nxt; (nxt = ssvh_raw_record_fastq(info.unmapped_raw, info.unmapped_bytes, off, &qname, &seq, &qual, &is_read1)) != 0; off = nxt) fn(qname, seq, qual, is_read1);
	}
	// the contig changes among the other records of the current batch (the flush sequence of clip_reads.h:423-438): fn(record index, new contig)
	template <class F> void contig_changes(const ssv_batch_t &b, int32_t &last_tid, F fn)
	{
		if (!on_device) {
			for (int64_t i = 0; i < b.n; ++i) {
				if (b.flag[i] & (4 | 8)) continue;
				if (b.tid[i] != last_tid) { last_tid = b.tid[i]; fn(i, last_tid); }
			}
			return;
		}
		for (uint32_t k = 0; k < info.n_tid_runs; ++k) { last_tid = info.tid_run_tid[k]; fn((int64_t)info.tid_run_index[k], last_tid); }
	}
	void contig_runs(const ssv_batch_t &b, int32_t &last_tid, vector<int32_t> &run_tids)
	{
		int32_t prev = last_tid;
		contig_changes(b, last_tid, [&](int64_t, int32_t tid) { run_tids.push_back(prev); prev = tid; });
	}
	void close()
	{
		if (reader.joinable()) {
			{ std::lock_guard<std::mutex> lk(mu); stop_reader = true; }
			cv.notify_all();
			reader.join();
		}
		if (announced >= cur && ctx) ssv_bamdec_prefetch_drop(ctx); // a chunk on its way that nobody will decode: its copy must have left the host pages
		for (Slot &S : slot) { if (S.reg_base) { ssv_host_unregister(S.reg_base); S.reg_base = nullptr; } stage_to_pool(S.stage); }
		if (text) { if (text->ctx) text->close(); delete text; text = nullptr; }
		if (bam) ssvh_bam_close(bam);
		bam = nullptr;
	}
};

static bool device_inflate_default() { const char *e = getenv("SSV_DEVICE_INFLATE"); return e && atoi(e) != 0; }

static vector<int> parse_devices(const char *s) // "-G 0,2,5"
{
	vector<int> d;
	for (const char *p = s; *p;) { d.push_back(atoi(p)); while (*p && *p != ',') ++p; if (*p == ',') ++p; }
	return d;
}

// GPU of rank r: the -G list (cycled) or the machine's GPUs in order (cycled: more ranks than GPUs is allowed - a one-GPU box runs every
// rank on its one GPU, one after the other in effect)
static int device_of_rank(int r, const vector<int> &devices)
{
	if (!devices.empty()) return devices[(size_t)r % devices.size()];
	const int n = ssv_device_count();
	return n > 0 ? r % n : 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// getclip
// ---------------------------------------------------------------------------------------------------------------------

// DisplaySClipReadsAndClipFq (clip_reads.h:300-345) for the clusters [k0, k1) of a table: their clip.gz rows and clip.fq records
// (the cluster table crosses PCIe in the compact format 3, include/seeksv_hip.h; the text written is the ASCII table's)
static int table_format_default() { return 3; }

// where a row's fields lie in the text (offsets: the strings still grow)
struct RowAt { uint32_t row, chr_len, cigar, cigar_len, aligned, aligned_len, clipped, clipped_len, cqual, cqual_len, fq; int32_t pos, support; char side; };
static void format_clusters(const ssv_cluster_table &t, ssvh_bam *bam, int64_t k0, int64_t k1, string &row, string &fq, vector<RowAt> *index = nullptr)
{
		row.reserve(row.size() + (size_t)(k1 - k0) * 480); fq.reserve(fq.size() + (size_t)(k1 - k0) * 200);
		if (row.empty()) ssv::thp_advise(row.data(), row.capacity()); // (tens of MB of text per thread and pass: on 2 MB pages where the kernel grants them, thp.h)
		if (fq.empty()) ssv::thp_advise(fq.data(), fq.capacity());
		char num[16];
		// (decimal digits by hand: three snprintf calls a row were a tenth of the formatter's time on a whole-genome sample's 5.5 M rows)
		auto put_int = [&num](long long v) -> size_t {
			char tmp[24]; size_t n = 0;
			const bool neg = v < 0;
			unsigned long long u = neg ? 0ull - (unsigned long long)v : (unsigned long long)v;
			do { tmp[n++] = (char)('0' + u % 10); u /= 10; } while (u);
			size_t o = 0;
			if (neg) num[o++] = '-';
			while (n) num[o++] = tmp[--n];
			return o;
		};
		string seqbuf;
		// a byte of the 2-bit base stream -> its four characters; of the 4-bit stream -> its two
		static const struct BaseTabs {
			uint32_t b2[256]; uint16_t b4[256];
			BaseTabs() {
				for (unsigned v = 0; v < 256; ++v) {
					char c[4];
					for (int i = 0; i < 4; ++i) c[i] = "ACGT"[(v >> (2 * i)) & 3];
					memcpy(&b2[v], c, 4);
					const char d[2] = {"=ACMGRSVTWYHKDBN"[v & 15], "=ACMGRSVTWYHKDBN"[v >> 4]};
					memcpy(&b4[v], d, 2);
				}
			}
		} base_tabs;
		std::vector<uint32_t> group_lut;   // grouped qualities: a group's number -> its (up to three) quality characters, as the low bytes of a dword
		const ssv_cluster_table *group_lut_for = nullptr;
		for (int64_t k = k0; k < k1; ++k) {
			const char *name = ssvh_bam_target_name(bam, t.tid[k]);
			const uint8_t *s = t.str + t.str_off[k];
			const size_t ll = (size_t)t.left_len[k], lr = (size_t)t.right_len[k];
			const char *sl, *ql, *sr, *qr;
			if (t.format == 3) { // compact: [base stream | quality stream] over seq_left + seq_right, whole 32-bit words each (seeksv_hip.h)
				const size_t n = ll + lr, W = (size_t)t.qual_bits, BBITS = (size_t)t.base_bits, QG = t.qual_group > 1 ? (size_t)t.qual_group : 1;
				const uint8_t *bs = s, *qs = s + 4 * ((n * BBITS + 31) / 32);
				seqbuf.resize(2 * n + 16); // (+ room for the whole dwords the table-driven loops write behind the last character)
				char *const sb = &seqbuf[0];
				if (BBITS == 2) {
					for (size_t i = 0, b = 0; i < n; i += 4, ++b) memcpy(sb + i, &base_tabs.b2[bs[b]], 4); // (the stream is whole dwords: the last byte is there)
					// the bases that are not A/C/G/T (sorted list; cluster << 28 | base index << 4 | code)
					const uint64_t *e0 = t.base_exc, *e1 = t.base_exc + t.n_base_exc;
					if (e0 != e1) for (const uint64_t *e = std::lower_bound(e0, e1, (uint64_t)k << 28); e < e1 && (*e >> 28) == (uint64_t)k; ++e) sb[(size_t)((*e >> 4) & 0xffffff)] = "=ACMGRSVTWYHKDBN"[*e & 15];
				} else for (size_t i = 0, b = 0; i < n; i += 2, ++b) memcpy(sb + i, &base_tabs.b4[bs[b]], 2);
				sl = sb; sr = sb + ll;
				if (W == 8) { ql = (const char *)qs; qr = ql + ll; }
				else if (QG > 1) { // groups of QG qualities: one number of W bits, its digits (radix = the alphabet's size) are the alphabet indices
					if (!group_lut_for || group_lut_for != &t) {
						unsigned radix = 0;
						while (radix < sizeof(t.qual_alphabet) && t.qual_alphabet[radix]) ++radix;
						group_lut.assign((size_t)1 << W, 0u);
						for (unsigned code = 0; code < (1u << W); ++code) { unsigned v = code; char c[4] = {0, 0, 0, 0}; for (size_t j = 0; j < 3; ++j) { c[j] = (char)t.qual_alphabet[radix ? v % radix : 0]; if (radix) v /= radix; } memcpy(&group_lut[code], c, 4); }
						group_lut_for = &t;
					}
					char *dq = sb + n;
					const unsigned mask = (1u << W) - 1u;
					const size_t ng = (n + QG - 1) / QG, qbytes = 4 * ((ng * W + 31) / 32);
					// (a group of up to 11 bits lies in at most three bytes: one unaligned dword from its first byte - read with bounds only for the stream's last three bytes)
					for (size_t g = 0; g < ng; ++g) {
						const size_t bit = g * W, b = bit >> 3;
						uint32_t w;
						if (b + 4 <= qbytes) memcpy(&w, qs + b, 4);
						else { w = 0; for (size_t x = b; x < qbytes; ++x) w |= (uint32_t)qs[x] << (8 * (x - b)); }
						const uint32_t chars = group_lut[(w >> (bit & 7)) & mask];
						memcpy(dq + g * QG, &chars, 4); // (the next group's characters overwrite the fourth byte; the last group's lands in the buffer's slack)
					}
					ql = dq; qr = dq + ll;
				} else {
					const unsigned mask = (1u << W) - 1u;
					char *dq = sb + n;
					const size_t qbytes = 4 * ((n * W + 31) / 32);
					for (size_t i = 0; i < n; ++i) { const size_t b = (i * W) >> 3; dq[i] = (char)t.qual_alphabet[((qs[b] | (b + 1 < qbytes ? (unsigned)qs[b + 1] << 8 : 0u)) >> ((i * W) & 7)) & mask]; }
					ql = dq; qr = dq + ll;
				}
			} else { sl = (const char *)s; ql = sl + ll; sr = sl + 2 * ll; qr = sl + 2 * ll + lr; }
			size_t lql = ll, lqr = lr;
			if (t.qual_missing[k]) { ql = qr = "*"; lql = lqr = 1; }
			RowAt at;
			at.row = (uint32_t)row.size(); at.fq = (uint32_t)fq.size(); at.pos = t.pos[k]; at.support = t.support[k]; at.side = (char)t.side[k];
			row += name ? name : ""; row += '\t';
			at.chr_len = (uint32_t)row.size() - 1 - at.row;
			row.append(num, put_int(t.pos[k])); row += '\t'; row += (char)t.side[k]; row += '\t';
			at.cigar = (uint32_t)row.size();
			for (int q = 0; q < t.n_cigar[k]; ++q) {
				const uint32_t op = t.cigar ? t.cigar[t.cigar_off[k] + q] : (uint32_t)reinterpret_cast<const uint16_t *>(t.c_cigar)[t.cigar_off[k] + q]; // (compact table: 16 bits an operation)
				if ((op & 15) == 4 || (op & 15) == 5) continue;
				row.append(num, put_int((long long)(op >> 4))); row += CIGAR_CHARS[op & 15];
			}
			at.cigar_len = (uint32_t)row.size() - at.cigar;
			row += '\t';
			at.aligned = (uint32_t)row.size();
			if (t.side[k] == '5') { at.aligned_len = (uint32_t)lr; at.clipped = at.aligned + (uint32_t)(lr + 1 + lqr + 1); at.clipped_len = (uint32_t)ll; at.cqual_len = (uint32_t)lql; }
			else { at.aligned_len = (uint32_t)ll; at.clipped = at.aligned + (uint32_t)(ll + 1 + lql + 1); at.clipped_len = (uint32_t)lr; at.cqual_len = (uint32_t)lqr; }
			at.cqual = at.clipped + at.clipped_len + 1;
			if (index) index->push_back(at);
			if (t.side[k] == '5') {
				row.append(sr, lr); row += '\t'; row.append(qr, lqr); row += '\t'; row.append(sl, ll); row += '\t'; row.append(ql, lql);
				fq += '@'; fq.append(sl, ll); fq += '\n'; fq.append(sl, ll); fq += "\n+\n"; fq.append(ql, lql); fq += '\n';
			} else {
				row.append(sl, ll); row += '\t'; row.append(ql, lql); row += '\t'; row.append(sr, lr); row += '\t'; row.append(qr, lqr);
				fq += '@'; fq.append(sr, lr); fq += '\n'; fq.append(sr, lr); fq += "\n+\n"; fq.append(qr, lqr); fq += '\n';
			}
			row += '\t'; row.append(num, put_int(t.support[k])); row += '\n';
		}
}

// `seeksv run`: a formatted piece's rows and FASTQ records as views into its text (the strings do not change any more)
static void index_piece(RunSession::Piece &p, const vector<RowAt> &ix)
{
	auto has_space = [](const char *q, size_t n) { for (size_t i = 0; i < n; ++i) if ((unsigned char)q[i] <= ' ') return true; return false; };
	const char *r = p.rows.data();
	p.parsed.reserve(ix.size()); p.reads.reserve(ix.size());
	if (p.rows.size() >= 0xffffffffull || p.fq.size() >= 0xffffffffull) p.clean = false;
	for (const RowAt &a : ix) {
		seeksv::ClipRow row;
		row.chr = seeksv::Str{r + a.row, a.chr_len}; row.pos = a.pos; row.side = a.side; row.cigar = seeksv::Str{r + a.cigar, a.cigar_len};
		row.aligned_seq = seeksv::Str{r + a.aligned, a.aligned_len}; row.clipped_seq = seeksv::Str{r + a.clipped, a.clipped_len}; row.clipped_qual = seeksv::Str{r + a.cqual, a.cqual_len};
		row.support = a.support;
		row.h = seeksv::clip_text_hash(row.clipped_seq.p, row.clipped_seq.n);
		// what `fin >> chr >> pos >> ...` (getsv.h:441-446) makes of the row's text: the same nine fields, unless one is empty or holds white space
		if (!a.chr_len || !a.cigar_len || !a.aligned_len || !a.clipped_len || !a.cqual_len || has_space(row.chr.p, row.chr.n)) p.clean = false;
		p.parsed.push_back(row);
		// the record's FASTQ text: '@' name '\n' sequence "\n+\n" qualities '\n' (clip_reads.h:320-321) - name = sequence
		p.reads.push_back(RunSession::FqRef{a.fq + 1 + a.clipped_len + 1, a.clipped_len, a.fq + 1 + a.clipped_len + 1 + a.clipped_len + 3, a.cqual_len});
	}
}

// A command's options AND operands, as its one parser made them of (argc, argv): the parser holds the command's optstring, prints its usage text and leaves
// with status 1 where the words are not a valid command line.  for_run: the words of `seeksv run -c / -v / -a` - options only, run fills in the operands
// (and what it decides itself) as fields.  What run must know to have been GIVEN, not defaulted, is a field too (`*_given`, an empty string).
struct GetclipOptions {
	double threshold = 0.9;
	int min_mapQ = 1, device = 0, n_ranks = 1, halo_bp = 65536;
	bool save_low_quality = false, device_inflate = device_inflate_default(), verify_crc = false, ranks_given = false, devices_given = false, prefix_given = false;
	bool mark_dups = false; // `run -M`, `somatic -K -M` (no option of getclip's own): duplicate read pairs are marked where the records are retained
	bool pair_dups = false; // `run -D`, `somatic -K -D` (no option of getclip's own): duplicate pairs by the unclipped 5' ends of both reads, marked once all records are retained
	bool sort_input = false; // `run -u` (no option of getclip's own): the input is in any order; its retained records are coordinate sorted on the GPU before any pass
	string regions_file;     // `run -L FILE` / `-X FILE`, `somatic -K -L` / `-X` (no option of getclip's own): the records that stay resident are restricted to a BED file's regions
	bool regions_exclude = false; // -X: a record stays iff it overlaps none of them
	bool splitread = false;  // `run -A` (no option of getclip's own): every decoded chunk also goes through the split-read scan, in front of retention, marks and restriction
	int splitread_mapq = 1;  // ... with getsv's -w as its MAPQ floor
	bool splitread_sa = false; // `run -A -S`: ... and a record that carries the read also gives a virtual candidate from its SA tag (ssv_rt_begin_original_sa)
	vector<int> devices;
	string prefix = "output", bamfile;
	void set_devices(const char *list) { devices = parse_devices(list); device = devices.empty() ? 0 : devices[0]; }
};

static GetclipOptions parse_getclip(int argc, char **argv, bool for_run = false)
{
	GetclipOptions o;
	int c;
	optind = 0; // (a fresh scan: nothing of the words scanned before is looked at again)
	while ((c = getopt(argc, argv, "t:q:o:sG:ZCN:H:")) >= 0) {
		switch (c) {
		case 't': o.threshold = atof(optarg); break;
		case 'q': o.min_mapQ = atoi(optarg); break;
		case 's': o.save_low_quality = true; break;
		case 'o': o.prefix = optarg; o.prefix_given = true; break;
		case 'G': o.set_devices(optarg); o.devices_given = true; break;
		case 'Z': o.device_inflate = true; break;
		case 'C': o.verify_crc = true; break;
		case 'N': o.n_ranks = atoi(optarg); o.ranks_given = true; break;
		case 'H': o.halo_bp = atoi(optarg); break;
		default: usage_getclip();
		}
	}
	if (argc != optind + (for_run ? 0 : 1) || o.n_ranks < 1 || o.halo_bp < 0) usage_getclip();
	if (!for_run) o.bamfile = argv[optind];
	return o;
}

// getclip's four outputs, created in the reference's order with its messages
struct ClipOutputs {
	GzOut soft, fq, unmapped1, unmapped2;
	explicit ClipOutputs(const string &prefix, bool create = true) // (create == false: a pass that writes nothing - nothing is opened, and nothing may be written or closed)
	{
		if (!create) return;
		const char *suffix[4] = {".clip.gz", ".clip.fq.gz", ".unmapped_1.fq.gz", ".unmapped_2.fq.gz"};
		GzOut *out[4] = {&soft, &fq, &unmapped1, &unmapped2};
		for (int k = 0; k < 4; ++k) if (!out[k]->open(prefix + suffix[k])) die("Cannot open file " + prefix + suffix[k]);
	}
	void close() { soft.close(); fq.close(); unmapped1.close(); unmapped2.close(); }
};

static ssv_clip_params clip_params(const GetclipOptions &o)
{
	ssv_clip_params p;
	memset(&p, 0, sizeof(p));
	p.match_rate = o.threshold; p.min_mapq = o.min_mapQ; p.save_low_quality = o.save_low_quality ? 1 : 0;
	return p;
}

static void rt_begin_for(const vector<string> &names, int min_mapq, ssv_ctx *ctx, bool original, bool sa = false); // (with the -F pass, below)

static int getclip_single(const GetclipOptions &o, RunSession *run)
{
	PhaseTimer pt;
	BatchSource src;
	const bool text_input = !is_bam_name(o.bamfile);
	// like the reference: complain about the input before anything is created (a text input's header is read here, and libbam's [samopen] line printed)
	// -L / -X: the BED file is read against the input's header here, so that a file that is refused leaves nothing behind
	const bool restrict = !o.regions_file.empty() && run && run->collect;
	const char *const restrict_opt = o.regions_exclude ? "-X" : "-L";
	seeksv::RegionList region_list;
	auto read_regions = [&](const ssvh_bam *header) {
		if (!restrict) return;
		vector<string> names;
		vector<int32_t> lens;
		for (int32_t t = 0, nt = ssvh_bam_n_targets(header); t < nt; ++t) { const char *nm = ssvh_bam_target_name(header, t); names.emplace_back(nm ? nm : ""); lens.push_back(ssvh_bam_target_len(header, t)); }
		string err;
		if (!seeksv::read_bed(o.regions_file, names, lens, region_list, &err)) die(err);
		if (region_list.unknown) cerr << "[seeksv] " << restrict_opt << ": " << region_list.unknown << " of " << region_list.lines << " lines of " << o.regions_file << " name a contig that the input's header does not have: ignored" << endl;
	};
	if (text_input) { src.open_text_header(o.bamfile, "[main_samview] fail to open file for reading."); read_regions(src.bam); }
	else {
		ssvh_bam *probe = nullptr;
		if (ssvh_bam_open(o.bamfile.c_str(), &probe) != 0) die("[main_samview] fail to open file for reading.");
		read_regions(probe);
		ssvh_bam_close(probe);
	}
	const bool probe_only = run && run->probe_only; // `somatic -K`, see RunSession
	ClipOutputs out(o.prefix, !probe_only);
	if (text_input) {
		std::unique_lock<std::shared_mutex> lk(g_outputs_mu);
		for (GzOut *g : {&out.soft, &out.fq, &out.unmapped1, &out.unmapped2}) g_outputs_unfinished.push_back(g->path);
	}
	const bool sort_input = o.sort_input && run && run->collect && !probe_only;
	if ((o.mark_dups && !probe_only) || sort_input || (o.pair_dups && run && run->collect && !probe_only)) { // -D: so does a sample whose rows and keys do not fit; -M: an input that is not coordinate sorted is refused where the stage meets it, and the run leaves no file behind; -u: so does a sample that does not fit twice
		std::unique_lock<std::shared_mutex> lk(g_outputs_mu);
		for (GzOut *g : {&out.soft, &out.fq, &out.unmapped1, &out.unmapped2}) g_outputs_refused.push_back(g->path);
	}

	const bool pair_dups = o.pair_dups && run && run->collect;
	src.any_order = sort_input;
	if (text_input && pair_dups) src.text->keep_all_seq = true;
	src.open(o.bamfile, [&] { return acquire_ctx(o.device, run); }, o.device_inflate, "[main_samview] fail to open file for reading.", run);
	ssv_ctx *ctx = src.ctx;
	ssv_clip_params p = clip_params(o);
	check(ctx, ssv_clip_begin(ctx, &p));
	ssv_clip_table_format(ctx, probe_only ? 0 : table_format_default()); // the compact table over PCIe; expanded by the formatting threads below (the probes read the ASCII table, and nobody reads its copy)
	ssvh_bam *bam = src.bam;
	if (run && text_input) { run->text_input = true; run->text_names = src.text->rd.target_names(); run->text_lens = src.text->rd.target_lens(); }
	pt.lap("open+gpu_init");

	// unmapped-pair side channel, StoreUnmapSeqAndQual (clip_reads.h:172-219): paired up, turned into FASTQ text and compressed by threads of its own
	// (unmapped_pairs.h); this thread hands every batch's raw UNMAP|MUNMAP records over by pointer
	auto keep_text = [run](int end, vector<string> &parts) { // (both sinks are called by one thread, and a piece is nobody's once it is written)
		if (run && run->keep_unmapped) for (string &s : parts) if (!s.empty()) run->unmapped[end].push_back(std::move(s));
	};
	seeksv::UnmappedPairs unmapped([&](vector<string> &parts) { out.unmapped1.write_parts(parts); keep_text(0, parts); }, [&](vector<string> &parts) { out.unmapped2.write_parts(parts); keep_text(1, parts); },
	                               std::max(1, std::min(8, ssv::effective_cpus() / 2)));
	// The flush sequence (clip_reads.h:428-438, :442): the reference writes out and clears its two maps at every change of contig among the
	// mapped-pair records.  A pass of the library bins by (contig, side, position), which is the same thing as long as every contig of the
	// pass is visited once, in ascending order - a coordinate-sorted BAM is ONE pass.  When a contig comes back (or one with a lower id
	// follows) the pass ends in front of that record (ssv_clip_scan_range), its rows go out, and the next pass starts there.
	vector<int32_t> pass_flushes;       // contigs flushed during the current pass, in order
	int32_t last_tid = 0, scan_last_tid = 0, pass_max_tid = 0; // (last_tid: the reader's side, one batch ahead of the scans)
	std::deque<vector<pair<int64_t, int32_t>>> changes_of; // per batch that was read and not yet scanned (the host reader runs one batch ahead)
	// The rows of a finished pass are formatted and compressed by a thread of their own while the main thread goes on reading and scanning the
	// next pass (the table sits in one of the context's two table sets: the emitter of pass k is joined before pass k + 1 is clustered, which is
	// when the library may touch that set again).  A coordinate-sorted BAM is one pass as far as the results go; it is cut at contig changes -
	// where the reference flushes anyway - whenever SSV_PASS_RECORDS records (default 16 M: about a contig of a 30x genome, so that only the last contig's rows are formatted after the last record) have gone into the pass, so that this overlap exists.
	static const int64_t pass_records_max = [] { const char *e = getenv("SSV_PASS_RECORDS"); return e ? std::max<int64_t>(1, atoll(e)) : (int64_t)16 << 20; }();
	int64_t pass_records = 0;
	std::thread emitter;
	double emit_format_s = 0, emit_gzip_s = 0;
	auto emit_pass = [&](bool last) {
		if (probe_only) { // the library runs the probes behind the table's kernels; the table itself is nobody's
			check(ctx, ssv_clip_cluster_async(ctx, nullptr, nullptr));
			pt.lap("gpu_cluster+probes");
			pass_flushes.clear();
			pass_records = 0;
			return;
		}
		if (emitter.joinable()) emitter.join();
		pt.lap("wait for the previous pass's output");
		ssv_cluster_table t;
		check(ctx, ssv_clip_cluster(ctx, &t));
		if (t.format == 3) check(ctx, ssv_clip_table_expand(ctx, &t, 0));
		pt.lap("gpu_cluster+table");
		// DisplaySClipReadsAndClipFq ('5' rows then '3' rows per contig run), clip_reads.h:300-345.  The rows of one cluster depend on nothing
		// else, so cluster ranges are formatted by several host threads and written out in order.
		int64_t k_end = 0;
		for (int32_t tid : pass_flushes) {
			const char *name = ssvh_bam_target_name(bam, tid);
			cerr << "Output merged soft-clipped reads of " << (name ? name : "") << endl;
			for (; k_end < t.n_clusters && t.tid[k_end] == tid; ++k_end) {}
		}
		pass_flushes.clear();
		pass_records = 0;
		emitter = std::thread([&, t, k_end] {
			const auto t0 = std::chrono::steady_clock::now();
			const int n_fmt = (int)std::max<int64_t>(1, std::min<int64_t>({(int64_t)ssv::effective_cpus(), 32, k_end / 4096}));
			vector<string> rows((size_t)n_fmt), fqs((size_t)n_fmt);
			const bool keep = run && run->collect; // `seeksv run`: the aligner step and the junction stage take these from memory
			vector<vector<RowAt>> index(keep ? (size_t)n_fmt : 0);
			auto format_range = [&](int w) {
				const int64_t k0 = k_end * w / n_fmt, k1 = k_end * (w + 1) / n_fmt;
				format_clusters(t, bam, k0, k1, rows[(size_t)w], fqs[(size_t)w], keep ? &index[(size_t)w] : nullptr);
			};
			{
				vector<std::thread> th;
				for (int w = 1; w < n_fmt; ++w) th.emplace_back(format_range, w);
				format_range(0);
				for (auto &x : th) x.join();
			}
			const auto t1 = std::chrono::steady_clock::now();
			out.soft.write_parts(rows); out.fq.write_parts(fqs);
			if (keep) {
				run->rows_kept = true;
				vector<RunSession::Piece *> fresh;
				vector<vector<RowAt> *> fresh_index;
				for (int w = 0; w < n_fmt; ++w) if (!rows[(size_t)w].empty()) {
					run->pieces.emplace_back();
					RunSession::Piece &p = run->pieces.back();
					p.rows = std::move(rows[(size_t)w]); p.fq = std::move(fqs[(size_t)w]);
					fresh.push_back(&p); fresh_index.push_back(&index[(size_t)w]);
				}
				{ // views and hashes, by as many threads as formatted (5.5 M rows of a whole-genome sample in all)
					vector<std::thread> th;
					for (size_t k = 1; k < fresh.size(); ++k) th.emplace_back([&, k] { index_piece(*fresh[k], *fresh_index[k]); });
					if (!fresh.empty()) index_piece(*fresh[0], *fresh_index[0]);
					for (auto &x : th) x.join();
				}
				if (run->on_pass) run->on_pass(fresh); // the aligner step starts on this pass's clipped sequences while the next pass is read
			}
			emit_format_s += std::chrono::duration<double>(t1 - t0).count();
			emit_gzip_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - t1).count();
		});
		if (last) { emitter.join(); pt.lap("wait for the last pass's output"); }
	};
	// -M: retention goes through ssv_dup_retain, which holds back a batch's trailing run: what it hands out is the records held back before, then the decoded
	// batch's up to its own trailing run.  The decoder's contig changes are relative to the decoded batch: they move by the records held back, and those that
	// fall into the new hold-back wait for the batch that brings their record (dup_pending: relative to the hold-back's first record).
	const bool mark_dups = o.mark_dups && run && run->collect;
	vector<ssv_batch_t> unsorted; // -u: the retained batches in input order
	static const char *const kSortNoMemory = "seeksv run: -u keeps the decoded sample in GPU memory twice while it is sorted (2 x 80 bytes a record, plus 24 bytes a record of keys): out of memory; "
	                                         "sort the input with `samtools sort` and run without -u";
	int64_t dup_held = 0;
	vector<pair<int64_t, int32_t>> dup_pending;
	if ((mark_dups || (o.pair_dups && run && run->collect)) && pt.on) ssv_prof_enable(ctx, 1); // (SSV_TIMING: the stage's own kernel time, below)
	if (mark_dups) check(ctx, ssv_dup_begin(ctx));
	// -L / -X: the list goes to the GPU once; every batch that stays passes through it directly behind retention and marking - in front of -u's sort and of every
	// scan -, and the contig changes that the scans get are those of the kept records (the call's own list), not the decoder's
	static const char *const kRegionNoMemory = "seeksv run: -L / -X write the kept records of a batch into memory of their own while the batch is still there: out of memory; "
	                                           "restrict the input with `samtools view -L` and run without the option";
	int32_t region_last_tid = 0;
	int64_t region_in = 0, region_kept = 0;
	if (restrict) {
		static_assert(sizeof(seeksv::Region) == sizeof(ssv_region), "the reader's triples are the library's");
		check(ctx, ssv_regions_set(ctx, reinterpret_cast<const ssv_region *>(region_list.regions.data()), (int64_t)region_list.regions.size(), ssvh_bam_n_targets(src.bam), o.regions_exclude ? 1 : 0));
		if (pt.on) ssv_prof_enable(ctx, 1);
	}
	auto region_changes = [&](const ssv_region_info &info, vector<pair<int64_t, int32_t>> &changes) {
		changes.clear();
		for (uint32_t k = 0; k < info.n_changes; ++k) changes.emplace_back((int64_t)info.change_index[k], info.change_tid[k]);
		region_last_tid = info.last_tid; region_in += info.n_in; region_kept += info.n_kept;
	};
	// a decoder's batch retained with the list applied (in the place of ssv_batch_retain), and a batch that is retained already restricted where it lies
	auto region_retain = [&](const ssv_batch_t &decoded, ssv_batch_t &b, vector<pair<int64_t, int32_t>> &changes) {
		ssv_region_info info;
		const int rc = ssv_region_retain(ctx, &decoded, region_last_tid, &b, &info);
		if (rc == SSV_E_NOMEM) die(probe_only ? "seeksv somatic -K: the normal's records do not fit this GPU's memory (80 bytes a record stay resident): out of memory; run `seeksv getclip` on the normal and `seeksv somatic` with its clip.gz instead" : kRegionNoMemory);
		check(ctx, rc);
		region_changes(info, changes);
	};
	auto region_select = [&](ssv_batch_t &b, vector<pair<int64_t, int32_t>> &changes) {
		ssv_region_info info;
		ssv_batch_t kept;
		const int rc = ssv_batch_select(ctx, &b, region_last_tid, &kept, &info);
		if (rc == SSV_E_NOMEM) die(kRegionNoMemory);
		check(ctx, rc);
		b = kept;
		region_changes(info, changes);
	};
	// the records of a retained (or decoded) batch through the clip scan, the pass ending in front of every contig that comes back
	auto scan_batch = [&](const ssv_batch_t &b, const vector<pair<int64_t, int32_t>> &changes) {
		int64_t lo = 0;
		for (const auto &ch : changes) {
			pass_flushes.push_back(scan_last_tid); // the visit that ends here is flushed
			if (ch.second <= pass_max_tid || pass_records + (ch.first - lo) >= pass_records_max) { // a contig that comes back (or a pass that is long enough): the pass ends in front of this record
				check(ctx, ssv_clip_scan_range(ctx, &b, lo, ch.first));
				emit_pass(false);
				p.initial_last_tid = scan_last_tid;
				check(ctx, ssv_clip_begin(ctx, &p));
				lo = ch.first;
			}
			pass_max_tid = scan_last_tid = ch.second;
		}
		check(ctx, ssv_clip_scan_range(ctx, &b, lo, b.n));
		pass_records += b.n - lo;
	};
	// -M: one call of ssv_dup_retain (decoded == nullptr: the end of the file, which flushes the hold-back) and the scan of what it handed out
	auto dup_step = [&](const ssv_batch_t *decoded, const vector<pair<int64_t, int32_t>> &changes) {
		ssv_batch_t none, b;
		memset(&none, 0, sizeof(none));
		none.mem = SSV_MEM_DEVICE;
		ssv_names_t names;
		memset(&names, 0, sizeof(names));
		names.mem = SSV_MEM_DEVICE;
		if (decoded) check(ctx, ssv_bamdec_names(ctx, &names));
		int64_t carried = 0;
		const int rc = ssv_dup_retain(ctx, decoded ? decoded : &none, &names, decoded ? 0 : 1, &b, &carried);
		if (rc == SSV_E_NOMEM && probe_only)
			die("seeksv somatic -K: the normal's records do not fit this GPU's memory (80 bytes a record stay resident): out of memory; run `seeksv getclip` on the normal and `seeksv somatic` with its clip.gz instead");
		check(ctx, rc);
		vector<pair<int64_t, int32_t>> now;
		vector<pair<int64_t, int32_t>> later;
		for (const auto &ch : dup_pending) (ch.first < b.n ? now : later).emplace_back(ch.first < b.n ? ch.first : ch.first - b.n, ch.second);
		for (const auto &ch : changes) { const int64_t at = dup_held + ch.first; (at < b.n ? now : later).emplace_back(at < b.n ? at : at - b.n, ch.second); }
		dup_pending.swap(later);
		dup_held += (decoded ? decoded->n : 0) - b.n;
		if (restrict) region_select(b, now); // (the flags are final: they came from the whole input)
		if (b.n == 0) { check(ctx, ssv_batch_release(ctx, &b)); return; } // (a batch that is one run entirely: its records come with a later one)
		run->batches.push_back(b);
		scan_batch(b, now);
	};
	// -D: the pump only retains (ssv_pairdup_retain: every batch with one row per record); one ssv_pairdup_mark behind the last chunk works on all of them, then
	// -u's sort where it was asked for, and then every batch goes through the clip scan - with the contig changes the decoder gave for it (pd_changes)
	vector<ssv_batch_t> pd_batches;
	vector<vector<pair<int64_t, int32_t>>> pd_changes;
	static const char *const kPairNoMemory = "seeksv run: -D keeps the decoded sample in GPU memory with 24 bytes a record of rows, and sorts 32 bytes a record that takes part: out of memory; "
	                                         "mark the duplicates beforehand and run without -D";
	static const char *const kProbeNoMemory = "seeksv somatic -K: the normal's records do not fit this GPU's memory (80 bytes a record stay resident): out of memory; run `seeksv getclip` on the normal and `seeksv somatic` with its clip.gz instead";
	// -A: the session is opened on this context and stays open behind the pass; every decoded chunk goes through its select (and what passes, through the gather)
	// before the chunk's batch is retained, marked, restricted or overwritten - ssv_rt_scan returns with the stream synchronised.  The decoders' default form
	// holds the bases of every record with S at an end, which is every record that carries the read: nothing more is decoded for it.
	const bool splitread = o.splitread && run && run->collect && !probe_only;
	if (splitread) {
		run->splitread_names.clear();
		for (int32_t t = 0, nt = ssvh_bam_n_targets(bam); t < nt; ++t) { const char *nm = ssvh_bam_target_name(bam, t); run->splitread_names.emplace_back(nm ? nm : ""); }
		rt_begin_for(run->splitread_names, o.splitread_mapq, ctx, true, o.splitread_sa);
		run->splitread_open = true; run->splitread_sa = o.splitread_sa;
		if (pt.on) ssv_prof_enable(ctx, 1);
	}
	auto splitread_scan = [&](const ssv_batch_t &decoded) {
		const auto t0 = std::chrono::steady_clock::now();
		ssv_names_t names;
		memset(&names, 0, sizeof(names));
		names.mem = SSV_MEM_DEVICE;
		if (text_input) names = src.text->names;
		else check(ctx, ssv_bamdec_names(ctx, &names));
		if (o.splitread_sa) { // -S: where the chunk's optional fields lie, asked of the decoder that made the chunk
			ssv_aux_t aux;
			check(ctx, text_input ? ssv_samdec_aux(ctx, &aux) : ssv_bamdec_aux(ctx, &aux));
			check(ctx, ssv_rt_scan_aux(ctx, &decoded, &names, &aux));
		} else check(ctx, ssv_rt_scan(ctx, &decoded, &names));
		run->splitread_scan_wall += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
		pt.lap("gpu_splitread_scan(wait kernels)");
	};
	src.pump(mark_dups || pair_dups ? 1 : 0, [&](const ssv_batch_t &b) {
		pt.lap(text_input ? "sam_read(wait)+gpu_decode" : o.device_inflate ? "bam_read(wait)+gpu_inflate+decode" : "bam_read(wait)");
		if (!probe_only) { const uint8_t *raw = nullptr; size_t raw_bytes = 0; src.unmapped_raw(&raw, &raw_bytes); unmapped.submit(raw, raw_bytes); }
		if (sort_input) { pt.lap("host_side_channel"); return; } // (-u: the contig changes are those of the sorted records, below)
		if (pair_dups) { // (kept until the scans, behind the mark)
			pd_changes.emplace_back();
			src.contig_changes(b, last_tid, [&](int64_t i, int32_t tid) { pd_changes.back().emplace_back(i, tid); });
			pt.lap("host_side_channel");
			return;
		}
		changes_of.emplace_back();
		src.contig_changes(b, last_tid, [&](int64_t i, int32_t tid) { changes_of.back().emplace_back(i, tid); });
		pt.lap("host_side_channel");
	}, [&](const ssv_batch_t &decoded) {
		if (splitread) splitread_scan(decoded);
		if (pair_dups) { // -D: the batch is only kept, with its rows; every pass waits for the mark
			ssv_names_t names;
			memset(&names, 0, sizeof(names));
			names.mem = SSV_MEM_DEVICE;
			if (text_input) names = src.text->names;
			else check(ctx, ssv_bamdec_names(ctx, &names));
			ssv_batch_t b;
			const int rc = ssv_pairdup_retain(ctx, &decoded, &names, &b);
			if (rc == SSV_E_NOMEM) die(probe_only ? kProbeNoMemory : kPairNoMemory); // (with -u too: what did not fit is -D's retention with rows)
			check(ctx, rc);
			(sort_input ? unsorted : pd_batches).push_back(b);
			pt.lap("gpu_retain+rows(wait h2d+kernels)");
			return;
		}
		if (sort_input) { // -u: the batch is only kept; every pass waits for the sort
			ssv_batch_t b;
			if (restrict) { // (the sort sees the kept records only)
				vector<pair<int64_t, int32_t>> unused;
				region_retain(decoded, b, unused);
				if (b.n == 0) check(ctx, ssv_batch_release(ctx, &b)); else unsorted.push_back(b);
				pt.lap("gpu_retain+regions(wait h2d+kernels)");
				return;
			}
			const int rc = ssv_batch_retain(ctx, &decoded, &b);
			if (rc == SSV_E_NOMEM) die(kSortNoMemory);
			check(ctx, rc);
			unsorted.push_back(b);
			pt.lap("gpu_retain(wait h2d+kernels)");
			return;
		}
		if (mark_dups) {
			dup_step(&decoded, changes_of.front());
			changes_of.pop_front();
			pt.lap("gpu_markdup+scan(wait h2d+kernels)");
			return;
		}
		ssv_batch_t b = decoded;
		if (restrict) { // -L / -X: only the kept records stay, and the scan gets their contig changes
			region_retain(decoded, b, changes_of.front());
			if (b.n == 0) check(ctx, ssv_batch_release(ctx, &b));
			else { run->batches.push_back(b); scan_batch(b, changes_of.front()); }
			changes_of.pop_front();
			pt.lap("gpu_regions+scan(wait h2d+kernels)");
			return;
		}
		if (run && run->collect) { // `seeksv run`: the batch stays in HBM for the getsv passes
			const int rc = ssv_batch_retain(ctx, &decoded, &b);
			if (rc == SSV_E_NOMEM && probe_only)
				die("seeksv somatic -K: the normal's records do not fit this GPU's memory (80 bytes a record stay resident): out of memory; run `seeksv getclip` on the normal and `seeksv somatic` with its clip.gz instead");
			check(ctx, rc);
			run->batches.push_back(b);
		}
		scan_batch(b, changes_of.front());
		changes_of.pop_front();
		pt.lap("gpu_scan(wait h2d+kernels)");
	});
	if (splitread && pt.on) { // (the later stages reset and switch the groups: the scans' time is read here)
		ssv_prof_get(ctx, o.splitread_sa ? "splitread_sa_scan" : "splitread_scan", &run->splitread_scan_ms, &run->splitread_scan_launches, nullptr);
		if (o.splitread_sa) ssv_prof_get(ctx, "splitread_sa_aux", &run->splitread_aux_ms, &run->splitread_aux_launches, nullptr);
		if (!(mark_dups || pair_dups || restrict)) ssv_prof_enable(ctx, 0);
	}
	if (mark_dups) { // the end of the file flushes the hold-back
		dup_step(nullptr, vector<pair<int64_t, int32_t>>());
		ssv_dup_stats ds;
		check(ctx, ssv_dup_finish(ctx, &ds));
		cerr << "[seeksv] -M: marked " << ds.heads_marked << " + " << ds.tails_marked << " duplicate records (" << ds.groups << " groups) of " << ds.records << endl;
		pt.lap("gpu_markdup(flush)");
		if (pt.on) {
			cerr << "[timing] (-M kernel time:";
			for (const char *g : {"dup_select", "dup_mark", "dup_retain"}) {
				double ms = 0; int64_t launches = 0;
				ssv_prof_get(ctx, g, &ms, &launches, nullptr);
				cerr << ' ' << g << ' ' << ms << " ms in " << launches << " launches" << (g[4] == 'r' ? "" : ",");
			}
			cerr << "; hold-back at most " << ds.held_max << " records, " << ds.set_entries << " digests in the set)" << endl;
			ssv_prof_enable(ctx, 0);
		}
	}
	if (pair_dups) { // -D: one mark over everything that was kept, in input order
		vector<ssv_batch_t> &kept = sort_input ? unsorted : pd_batches;
		ssv_pairdup_stats ps;
		const int rc = ssv_pairdup_mark(ctx, kept.data(), (int64_t)kept.size(), &ps);
		if (rc == SSV_E_NOMEM) die(probe_only ? kProbeNoMemory : kPairNoMemory);
		check(ctx, rc);
		cerr << "[seeksv] -D: marked " << ps.pairs_marked << " duplicate pairs (" << ps.groups_many << " groups of two or more) of " << ps.pairs << " pairs; " << ps.unpaired << " of " << ps.taking_part
		     << " records that take part have no mate by name, " << ps.records << " records" << endl;
		pt.lap("gpu_pair_duplicates");
		if (pt.on) {
			cerr << "[timing] (-D kernel time:";
			const char *const groups[3] = {"pairdup_ends", "pairdup_join", "pairdup_mark"};
			for (int k = 0; k < 3; ++k) {
				double ms = 0; int64_t launches = 0;
				ssv_prof_get(ctx, groups[k], &ms, &launches, nullptr);
				cerr << ' ' << groups[k] << ' ' << ms << " ms in " << launches << " launches" << (k == 2 ? ";" : ",");
			}
			cerr << " resident at the peak beside the records: " << 24 * ps.records << " bytes of rows, " << 8 * ps.records + 32 * ps.taking_part + 32 * ps.pairs << " bytes of keys and indices)" << endl;
			ssv_prof_enable(ctx, restrict ? 1 : 0); // (-L / -X: the selects below are timed too)
		}
		if (restrict && sort_input) { // (the marked batches, restricted in front of the sort)
			vector<ssv_batch_t> still;
			vector<pair<int64_t, int32_t>> unused;
			for (ssv_batch_t &b : unsorted) {
				region_select(b, unused);
				if (b.n == 0) check(ctx, ssv_batch_release(ctx, &b)); else still.push_back(b);
			}
			unsorted.swap(still);
			pt.lap("gpu_regions");
		}
		if (!sort_input) {
			for (size_t k = 0; k < pd_batches.size(); ++k) {
				ssv_batch_t b = pd_batches[k];
				if (restrict) region_select(b, pd_changes[k]);
				if (b.n == 0) { check(ctx, ssv_batch_release(ctx, &b)); continue; }
				run->batches.push_back(b);
				scan_batch(b, pd_changes[k]);
				pt.lap("gpu_scan(wait kernels)");
			}
			pd_batches.clear();
		}
	}
	if (sort_input) { // -u: one sort of everything that was kept; then the passes see the batches as they would have come from a sorted file
		if (pt.on) { ssv_prof_enable(ctx, 1); if (!restrict) ssv_prof_reset(ctx); } // (-L / -X: the region groups' time so far stays; the sort's groups are its own)
		const size_t n_unsorted = unsorted.size();
		auto resident = [](const ssv_batch_t *b, int64_t n) { // hot columns, cigar_ends, lines, operations, bases + qualities
			int64_t bytes = 0;
			for (int64_t k = 0; k < n; ++k) bytes += b[k].n * (4 + 4 + 2 + 1 + 64) + b[k].n_cigar_total * 4 + b[k].seqqual_bytes;
			return bytes;
		};
		int64_t bytes_in = resident(unsorted.data(), (int64_t)n_unsorted);
		if (pair_dups) for (const ssv_batch_t &b : unsorted) bytes_in += 24 * b.n; // (-D: the inputs still carry their rows, dead since the mark)
		ssv_sorted sorted;
		const int rc = ssv_batch_sort(ctx, unsorted.data(), (int64_t)n_unsorted, ssvh_bam_n_targets(bam), 0, &sorted);
		if (rc == SSV_E_NOMEM) die(kSortNoMemory);
		check(ctx, rc);
		unsorted.clear(); // (the call's: released, or handed back as the result's batches)
		if (sorted.already_sorted) cerr << "[seeksv] -u: " << sorted.n_records << " records in " << sorted.n_batches << " batches already in coordinate order" << endl;
		else cerr << "[seeksv] -u: sorted " << sorted.n_records << " records from " << n_unsorted << " into " << sorted.n_batches << " batches" << endl;
		pt.lap("gpu_coordinate_sort");
		if (pt.on) {
			cerr << "[timing] (-u kernel time:";
			for (const char *g : {"sort_keys", "sort_radix", "sort_gather"}) {
				double ms = 0; int64_t launches = 0;
				ssv_prof_get(ctx, g, &ms, &launches, nullptr);
				cerr << ' ' << g << ' ' << ms << " ms in " << launches << " launches" << (g[5] == 'g' ? ";" : ",");
			}
			const int64_t bytes_out = sorted.already_sorted ? 0 : resident(sorted.batches, sorted.n_batches), bytes_keys = sorted.already_sorted ? 0 : 24 * sorted.n_records;
			cerr << " resident at the peak: " << bytes_in << " + " << bytes_out << " bytes of records, " << bytes_keys << " bytes of keys and indices)" << endl;
			ssv_prof_enable(ctx, 0);
		}
		for (int64_t k = 0; k < sorted.n_batches; ++k) {
			const ssv_batch_t &b = sorted.batches[k];
			if (b.n == 0) { ssv_batch_t gone = b; check(ctx, ssv_batch_release(ctx, &gone)); continue; }
			vector<pair<int64_t, int32_t>> changes;
			for (int64_t j = sorted.change_first[k]; j < sorted.change_first[k + 1]; ++j) changes.emplace_back((int64_t)sorted.change_index[j], sorted.change_tid[j]);
			run->batches.push_back(b);
			scan_batch(b, changes);
			pt.lap("gpu_scan(wait kernels)");
		}
	}
	if (restrict) {
		cerr << "[seeksv] " << restrict_opt << ": kept " << region_kept << " of " << region_in << " records (" << region_list.regions.size() << " regions on " << region_list.contigs << " contigs)" << endl;
		if (pt.on) {
			cerr << "[timing] (" << restrict_opt << " kernel time:";
			const char *const groups[2] = {"region_select", "region_gather"};
			for (int k = 0; k < 2; ++k) {
				double ms = 0; int64_t launches = 0;
				ssv_prof_get(ctx, groups[k], &ms, &launches, nullptr);
				cerr << ' ' << groups[k] << ' ' << ms << " ms in " << launches << " launches" << (k == 1 ? ")" : ",");
			}
			cerr << endl;
		}
		check(ctx, ssv_regions_clear(ctx)); // (the stage's memory goes back in front of the passes that follow)
	}
	pass_flushes.push_back(scan_last_tid);
	emit_pass(true);
	if (!probe_only) cerr << "[GetSClipReads] finished!" << endl;
	unmapped.finish();
	if (!probe_only) out.close();
	{ std::unique_lock<std::shared_mutex> lk(g_outputs_mu); g_outputs_unfinished.clear(); g_outputs_refused.clear(); }
	pt.lap("gzip");
	if (pt.on) cerr << "[timing] (unmapped side channel, beside the reading: " << unmapped.records() << " records, " << unmapped.pairs() << " pairs written, its thread busy " << unmapped.busy_seconds() << " s)" << endl;
	if (pt.on) cerr << "[timing] (format, all passes, beside the reading: " << emit_format_s << " s; gzip: " << emit_gzip_s << " s)" << endl;
	src.close();
	release_ctx(ctx, run);
	pt.lap("teardown");
	return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// getclip over N runs of records, one per GPU (-N): the file is cut at record starts (ssvh_bam_partition); a rank scans its run plus the
// halo of records before it that can own a breakpoint inside it, keeps the clip events whose breakpoint lies in its interval, and clusters
// them: every (contig, side, position) bin lives on exactly one rank with its reads in file order, so the tables need no exchange - the
// rows are put together per contig: the '5' rows of all ranks in rank order, then the '3' rows (clip_reads.h:432-433).
// ---------------------------------------------------------------------------------------------------------------------

struct UnmappedRec { string qname, seq, qual; int is_read1; };

struct ClipRank {
	vector<int32_t> run_tids;                       // contig runs among the rank's own mapped-pair records
	int32_t last_tid = 0;
	vector<UnmappedRec> unmapped;                   // UNMAP|MUNMAP records of the rank's own run, in file order
	map<pair<int32_t, char>, pair<string, string>> seg; // (contig, side) -> rows, fastq records
	int32_t max_span = 0;
	string err;
};

static int getclip_ranks(const GetclipOptions &o, RunSession *run)
{
	PhaseTimer pt;
	ssvh_bam *bam = nullptr;
	if (ssvh_bam_open(o.bamfile.c_str(), &bam) != 0) die("[main_samview] fail to open file for reading.");
	ClipOutputs files(o.prefix);
	vector<ssvh_bam_part> parts((size_t)o.n_ranks);
	if (ssvh_bam_partition(o.bamfile.c_str(), o.n_ranks, o.halo_bp, parts.data()) != 0) die(string("[seeksv] ") + ssvh_partition_last_error());
	pt.lap("open+partition");
	const int32_t n_targets = ssvh_bam_n_targets(bam);
	vector<ClipRank> R((size_t)o.n_ranks);
	// `seeksv run -N`: the ranks' contexts and the records of their own runs outlive this function
	RunRanks *const keep = run && !run->ranks.rank.empty() ? &run->ranks : nullptr;
	if (keep) keep->parts = parts;
	auto rank_main = [&](int r) {
		ClipRank &out = R[(size_t)r];
		const ssvh_bam_part &P = parts[(size_t)r];
		ssv_ctx *ctx = keep ? keep->rank[(size_t)r].ctx : nullptr;
		if (!ctx && ssv_ctx_create(device_of_rank(r, o.devices), &ctx) != SSV_OK) { out.err = string("[seeksv] ") + ssv_last_error(nullptr); return; }
		if (keep) keep->rank[(size_t)r].ctx = ctx;
		auto drop_ctx = [&] { if (!keep) ssv_ctx_destroy(ctx); }; // (kept: the run lets go of it)
		ssv_clip_params p = clip_params(o);
		// breakpoints (contig, 1-based position) owned by this rank: from its first record's 0-based start taken as a 1-based position - the
		// smallest key a record can give (a '5' event sits at start + 1, a '3' event at start + reference span, and the span is 0 for a CIGAR
		// that is one lone soft clip, clip_reads.cpp:150-190) - up to the next rank's
		p.use_ownership = 1; p.initial_last_tid = P.initial_last_tid;
		p.own_lo_tid = r == 0 ? 0 : P.own_tid; p.own_lo_pos = r == 0 ? 0 : P.own_pos;
		if (r + 1 < o.n_ranks) { p.own_hi_tid = parts[(size_t)r + 1].own_tid; p.own_hi_pos = parts[(size_t)r + 1].own_tid < n_targets ? parts[(size_t)r + 1].own_pos : 0; }
		else { p.own_hi_tid = INT32_MAX; p.own_hi_pos = 0; }
		if (ssv_clip_begin(ctx, &p) != SSV_OK) { out.err = string("[seeksv] ") + ssv_last_error(ctx); drop_ctx(); return; }
		ssv_clip_table_format(ctx, table_format_default());
		ssvh_bam *rb = nullptr; // (the header: contig names for the rows)
		if (ssvh_bam_open(o.bamfile.c_str(), &rb) != 0) { out.err = "[main_samview] fail to open file for reading."; drop_ctx(); return; }
		// the contig of the last mapped-pair record before the rank's OWN run (its run list continues from there)
		out.last_tid = r == 0 ? 0 : P.before_own_tid;
		for (int phase = 0; phase < 2 && out.err.empty(); ++phase) { // 0: the halo (scanned, nothing else), 1: the rank's own records
			if (phase == 0 && P.scan_coff == P.own_coff && P.scan_uoff == P.own_uoff) continue;
			BatchSource src; // host threads or the GPU (-Z) inflate and decode the run's blocks
			if (phase == 0) src.set_range(P.scan_coff, P.scan_uoff, P.own_coff, P.own_uoff);
			else { src.set_range(P.own_coff, P.own_uoff, P.end_coff, P.end_uoff); src.r_prev_tid = out.last_tid; }
			src.open(o.bamfile, ctx, o.device_inflate, "[main_samview] fail to open file for reading.");
			src.pump(0, [&](const ssv_batch_t &b) {
				out.max_span = std::max(out.max_span, b.max_ref_span);
				if (phase != 1) return;
				src.for_each_unmapped([&](const char *qname, const char *seq, const char *qual, int is_read1) { out.unmapped.push_back(UnmappedRec{qname, seq, qual, is_read1}); });
				src.contig_runs(b, out.last_tid, out.run_tids);
			}, [&](const ssv_batch_t &decoded) {
				if (!out.err.empty()) return;
				ssv_batch_t b = decoded;
				if (keep && phase == 1) { // the rank's own records stay in its GPU's memory for the getsv pass
					if (ssv_batch_retain(ctx, &decoded, &b) != SSV_OK) { out.err = string("[seeksv] ") + ssv_last_error(ctx); return; }
					keep->rank[(size_t)r].batches.push_back(b); keep->rank[(size_t)r].kept += b.n;
				}
				if (ssv_clip_scan(ctx, &b) != SSV_OK) out.err = string("[seeksv] ") + ssv_last_error(ctx);
			});
			src.close();
		}
		ssv_cluster_table t;
		if (out.err.empty() && ssv_clip_cluster(ctx, &t) != SSV_OK) out.err = string("[seeksv] ") + ssv_last_error(ctx);
		if (out.err.empty() && t.format == 3 && ssv_clip_table_expand(ctx, &t, 2) != SSV_OK) out.err = string("[seeksv] ") + ssv_last_error(ctx);
		if (out.err.empty()) {
			for (int64_t k0 = 0; k0 < t.n_clusters;) { // the table is in (contig, side, position) order
				int64_t k1 = k0;
				while (k1 < t.n_clusters && t.tid[k1] == t.tid[k0] && t.side[k1] == t.side[k0]) ++k1;
				auto &sg = out.seg[make_pair(t.tid[k0], (char)t.side[k0])];
				format_clusters(t, rb, k0, k1, sg.first, sg.second);
				k0 = k1;
			}
		}
		ssvh_bam_close(rb);
		drop_ctx();
	};
	{
		vector<std::thread> th;
		for (int r = 1; r < o.n_ranks; ++r) th.emplace_back(rank_main, r);
		rank_main(0);
		for (auto &x : th) x.join();
	}
	pt.lap("ranks(scan+cluster+format)");
	int32_t max_span = 0;
	for (auto &o : R) { if (!o.err.empty()) die(o.err); max_span = std::max(max_span, o.max_span); }
	if (max_span > o.halo_bp) die("[seeksv] a read spans " + to_string(max_span) + " reference bases, more than the halo of " + to_string(o.halo_bp) + " bp before a run of records: rerun with -H " + to_string(max_span));
	// the flush sequence of the whole file: the ranks' run lists one after the other (a rank's list continues the previous rank's)
	vector<int32_t> run_tids;
	for (auto &o : R) run_tids.insert(run_tids.end(), o.run_tids.begin(), o.run_tids.end());
	int32_t last_tid = 0;
	for (int r = o.n_ranks - 1; r >= 0; --r) if (parts[(size_t)r].own_coff != UINT64_MAX || r == 0) { last_tid = R[(size_t)r].last_tid; break; }
	run_tids.push_back(last_tid);
	for (size_t k = 1; k < run_tids.size(); ++k)
		if (run_tids[k] <= run_tids[k - 1]) {
			// Contigs that come back: the ranks' intervals of (contig, position) mean nothing for such a file.  The reference's result - one
			// flush per visit of a contig (clip_reads.h:428-438) - comes from the single-GPU path, which ends a pass at every such visit.
			ssvh_bam_close(bam);
			if (keep) { // `seeksv run -N`: from here on the run is `seeksv run` on the first device - one context, which keeps every record
				run->fall_back();
				cerr << "[seeksv] run -N: contigs come back in " << o.bamfile << ", the ranks give way to one GPU (as `seeksv run` without -N)" << endl;
			}
			GetclipOptions single = o;
			single.device = device_of_rank(0, o.devices);
			return getclip_single(single, run);
		}
	// unmapped-pair side channel, StoreUnmapSeqAndQual (clip_reads.h:172-219): sequential over the file, i.e. over the ranks in order
	map<string, pair<pair<string, string>, char>> id2seq_qual;
	for (auto &o : R) for (auto &u : o.unmapped) {
		auto it = id2seq_qual.find(u.qname);
		if (it != id2seq_qual.end()) {
			if (u.is_read1 && it->second.second == '2') {
				files.unmapped1.write(string("@") + it->first + "/1\n" + u.seq + "\n+\n" + u.qual + "\n");
				files.unmapped2.write(string("@") + it->first + "/2\n" + it->second.first.first + "\n+\n" + it->second.first.second + "\n");
				id2seq_qual.erase(it);
			} else if (!u.is_read1 && it->second.second == '1') {
				files.unmapped1.write(string("@") + it->first + "/1\n" + it->second.first.first + "\n+\n" + it->second.first.second + "\n");
				files.unmapped2.write(string("@") + it->first + "/2\n" + u.seq + "\n+\n" + u.qual + "\n");
				id2seq_qual.erase(it);
			}
		} else id2seq_qual.insert(make_pair(u.qname, make_pair(make_pair(u.seq, u.qual), u.is_read1 ? '1' : '2')));
	}
	vector<string> rows, fqs;
	for (int32_t tid : run_tids) {
		const char *name = ssvh_bam_target_name(bam, tid);
		cerr << "Output merged soft-clipped reads of " << (name ? name : "") << endl;
		for (char side : {'5', '3'})
			for (auto &o : R) {
				auto it = o.seg.find(make_pair(tid, side));
				if (it == o.seg.end()) continue;
				rows.push_back(std::move(it->second.first)); fqs.push_back(std::move(it->second.second));
			}
	}
	files.soft.write_parts(rows); files.fq.write_parts(fqs);
	cerr << "[GetSClipReads] finished!" << endl;
	files.close();
	pt.lap("output");
	ssvh_bam_close(bam);
	return 0;
}

static int getclip_main(const GetclipOptions &o, RunSession *run)
{
	if (o.verify_crc) g_verify_crc = true;
	if (o.n_ranks > 1 && !is_bam_name(o.bamfile)) die("seeksv getclip: -N cuts a BAM into runs of records; SAM text is read once, from its start to its end, by one GPU");
	return o.n_ranks > 1 ? getclip_ranks(o, run) : getclip_single(o, run);
}

static int cmd_getclip(int argc, char **argv) { return getclip_main(parse_getclip(argc, argv), nullptr); }

// ---------------------------------------------------------------------------------------------------------------------
// getsv (junctions from -B)
// ---------------------------------------------------------------------------------------------------------------------

static string cigar_text(const SeqInfo &s) // DisplayCigarVector, clip_reads.h:489-505
{
	string o;
	if (s.left_clipped > 0) o += to_string(s.left_clipped) + "S";
	for (auto &pr : s.cigar_vec) { o += to_string(pr.first); o += pr.second; }
	if (s.right_clipped > 0) o += to_string(s.right_clipped) + "S";
	return o;
}

static string sv_type(const Junction &j) // GetSVType, clip_reads.cpp:572-581
{
	if (j.up_chr != j.down_chr) return "CTX";
	if (j.up_strand != j.down_strand) return "INV";
	if (j.up_pos < j.down_pos) return "DEL";
	if (j.up_pos > j.down_pos) return "INS";
	return "Unknown";
}

static double largest_base_frequency(const string &seq) // CountLargestBaseFrequency, getsv.cpp:1485
{
	int a = 0, t = 0, c = 0, g = 0, n = 0;
	for (char ch : seq) {
		if (ch == 'A' || ch == 'a') ++a; else if (ch == 'T' || ch == 't') ++t; else if (ch == 'C' || ch == 'c') ++c; else if (ch == 'G' || ch == 'g') ++g; else ++n;
	}
	int largest = max(max(max(a, t), max(c, g)), n);
	return largest / (double)seq.length();
}

// CalculateInsertsizeDeviation (cluster.cpp:15-83) over the head of a BAM, with the reference's stderr lines
// CalculateInsertsizeDeviation (cluster.cpp:15-83) reads the file until it has its pairs - the first chunk or the first few.  With the records decoded on the
// GPU their batches are copied into memory that stays (ssv_batch_retain; resident ones stay anyway): `keep` then holds the open source and those batches, and the
// fused pass scans them and goes on from the next chunk instead of reading, inflating and decoding the head of the file again.
struct IsizeCarry {
	BatchSource src; vector<ssv_batch_t> kept; bool owned = false, usable = false;
	void drop(ssv_ctx *ctx) { if (usable) { if (owned) for (auto &k : kept) ssv_batch_release(ctx, &k); kept.clear(); src.close(); usable = false; } } // the pass that went on from it is over, or there was none
};

static void insert_size_pass(const std::function<ssv_ctx *()> &get_ctx, const string &bamfile, bool device_inflate, int min_mapQ, int read_pair_used, int &mean_insert_size, int &deviation, IsizeCarry *keep,
                             const RunSession *run, string *report = nullptr) // report: the pass's stderr lines go there instead (a caller that has earlier lines still to print)
{
	BatchSource local;
	BatchSource &src = keep ? keep->src : local;
	src.open(bamfile, get_ctx, device_inflate, "[main_samview] fail to open file for reading.", run);
	ssv_ctx *ctx = src.ctx ? src.ctx : get_ctx();
	ssv_isize_begin(ctx, min_mapQ, read_pair_used);
	int32_t done = 0;
	int chunks = 0;
	ssv_batch_t b;
	memset(&b, 0, sizeof(b));
	while (!done) {
		if (!src.next(&b, 0)) break;
		++chunks;
		check(ctx, ssv_isize_accumulate(ctx, &b, &done));
		if (keep && src.on_device) { // a decoder's batch is valid until the next decode: a copy that stays (80 B/record, device to device)
			ssv_batch_t k = b;
			if (!src.resident) { check(ctx, ssv_batch_retain(ctx, &b, &k)); keep->owned = true; }
			keep->kept.push_back(k);
		}
	}
	int64_t n; int32_t m = 0, sd = 0;
	ssv_isize_finish(ctx, &n, &m, &sd);
	if (n > 0) {
		mean_insert_size = m; deviation = sd;
		std::ostringstream o;
		o << "Bam/sam " << bamfile << "    Mean insert size : " << mean_insert_size << "\n" << "Mean deviation: " << deviation << "\n";
		if (report) *report += o.str(); else { cerr << o.str(); cerr.flush(); }
	}
	if (keep && src.on_device && chunks >= 1) { keep->usable = true; return; }
	src.close();
}

static void resident_alignments(const RunSession &run, seeksv::AlnRecords &R); // `seeksv run`: the aligner step's records as the join reads them

// getsv -F: FindJunction (process_bwasw.cpp:5-227).  A name that ends in ".bam" is BAM, every other name SAM text (the reference's rule, process_bwasw.cpp:12-16).
// A BAM goes through the same readers as the original BAM (host threads, or the GPU with -Z); SAM text is always parsed on the GPU (ssv_samdec_*), whatever -Z
// says.  Selection, pairing by read name and the junction of every pair run on the GPU (ssv_rt_*), the pairs are applied to the map here in their order.
static const char *kRtOpenError = "[main_samview] fail to open file for reading.";

static void rt_begin_for(const vector<string> &names, int min_mapq, ssv_ctx *ctx, bool original, bool sa)
{
	const int32_t nt = (int32_t)names.size();
	// contigs in byte-wise name order: the device compares (rank, pos) where the reference compares make_pair(chr, pos)
	vector<int32_t> order((size_t)nt), rank((size_t)nt);
	for (int32_t t = 0; t < nt; ++t) order[(size_t)t] = t;
	std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return names[(size_t)a] < names[(size_t)b]; });
	for (int32_t k = 0; k < nt; ++k) rank[(size_t)order[(size_t)k]] = k;
	ssv_rt_params rp;
	memset(&rp, 0, sizeof(rp));
	rp.min_mapq = min_mapq; rp.n_targets = nt; rp.name_rank = rank.data();
	if (sa) { // -S: the SA entries name contigs, which the session looks up
		vector<const char *> ptrs((size_t)nt + 1, nullptr);
		for (int32_t t = 0; t < nt; ++t) ptrs[(size_t)t] = names[(size_t)t].c_str();
		check(ctx, ssv_rt_begin_original_sa(ctx, &rp, ptrs.data()));
		return;
	}
	check(ctx, original ? ssv_rt_begin_original(ctx, &rp) : ssv_rt_begin(ctx, &rp));
}

static void sam_text_pass(const string &path, ssv_ctx *ctx, vector<string> &names, const std::function<void()> &begin,
                          const std::function<void(const ssv_batch_t &, const ssv_names_t &)> &on_batch)
{
	SamTextDecoder d;
	d.open(path, kRtOpenError);
	names = d.rd.target_names();
	begin();
	d.begin(ctx, false);
	ssv_batch_t b;
	while (d.next(&b)) if (b.n) on_batch(b, d.names);
	d.close();
}

// the -F file as SAM text
static void readthrough_pass_sam(const string &path, int min_mapq, ssv_ctx *ctx, vector<string> &names)
{
	sam_text_pass(path, ctx, names, [&] { rt_begin_for(names, min_mapq, ctx, false); },
	              [&](const ssv_batch_t &b, const ssv_names_t &nm) { check(ctx, ssv_rt_scan(ctx, &b, &nm)); });
}

// The re-alignments of the clipped sequences as SAM text (`bwa mem ref.fa out.clip.fq.gz > out.clip.sam`, or piped in: getsv.h:437-446 opens every name
// without ".bam" as text): decoded on the GPU chunk by chunk, every batch packed there into the columns the join reads (ssv_aln_pack: fixed fields, names back
// to back, their hashes) and appended here; offsets are rebased by the running totals.
struct ClipAlignments {
	vector<int32_t> tid, pos;
	vector<uint16_t> flag, n_cigar;
	vector<uint8_t> mapq;
	vector<uint32_t> cigar_off, cigar;
	vector<uint64_t> name_off, hash;
	vector<char> names;
	vector<const char *> qname;
	seeksv::AlnRecords R;
};

static void clip_sam_pass(const string &path, ssv_ctx *ctx, ClipAlignments &A)
{
	sam_text_pass(path, ctx, A.R.target_names, [] {}, [&](const ssv_batch_t &b, const ssv_names_t &nm) {
		ssv_aln_cols c;
		check(ctx, ssv_aln_pack(ctx, &b, &nm, &c));
		const size_t n = (size_t)c.n, n0 = A.tid.size(), ops0 = A.cigar.size(), bytes0 = A.names.size();
		if (ops0 + (size_t)c.n_cigar_total >= ((size_t)1 << 32)) die("[seeksv] more than 2^32 CIGAR operations among the clipped-sequence alignments");
		A.tid.insert(A.tid.end(), c.tid, c.tid + n); A.pos.insert(A.pos.end(), c.pos, c.pos + n);
		A.flag.insert(A.flag.end(), c.flag, c.flag + n); A.n_cigar.insert(A.n_cigar.end(), c.n_cigar, c.n_cigar + n);
		A.mapq.insert(A.mapq.end(), c.mapq, c.mapq + n); A.hash.insert(A.hash.end(), c.name_hash, c.name_hash + n);
		A.cigar.insert(A.cigar.end(), c.cigar, c.cigar + c.n_cigar_total);
		A.names.insert(A.names.end(), c.names, c.names + c.name_bytes);
		A.cigar_off.resize(n0 + n); A.name_off.resize(n0 + n);
		for (size_t i = 0; i < n; ++i) { A.cigar_off[n0 + i] = c.cigar_off[i] + (uint32_t)ops0; A.name_off[n0 + i] = c.name_off[i] + bytes0; }
	});
	const size_t n = A.tid.size();
	A.qname.resize(n);
	for (size_t i = 0; i < n; ++i) A.qname[i] = A.names.data() + A.name_off[i];
	seeksv::AlnRecords &R = A.R;
	R.n = (int64_t)n; R.tid = A.tid.data(); R.pos = A.pos.data(); R.flag = A.flag.data(); R.n_cigar = A.n_cigar.data(); R.mapq = A.mapq.data();
	R.cigar_off = A.cigar_off.data(); R.cigar = A.cigar.data(); R.qname = A.qname.data(); R.qhash = A.hash.data();
}

static void readthrough_pass(const string &path, int min_mapq, ssv_ctx *ctx, bool device_inflate, JunctionMap &junction2other)
{
	vector<string> names;
	if (!is_bam_name(path)) readthrough_pass_sam(path, min_mapq, ctx, names);
	else {
		ssvh_bam *hdr = nullptr;
		if (ssvh_bam_open(path.c_str(), &hdr) != 0) die(kRtOpenError);
		const int32_t nt = ssvh_bam_n_targets(hdr);
		names.resize((size_t)nt);
		for (int32_t t = 0; t < nt; ++t) { const char *z = ssvh_bam_target_name(hdr, t); names[(size_t)t] = z ? z : ""; }
		ssvh_bam_close(hdr);
		rt_begin_for(names, min_mapq, ctx, false);
		BatchSource src;
		src.any_order = true; // (a bwasw file is in read order, not coordinate order)
		src.open(path, ctx, device_inflate, kRtOpenError);
		if (!src.on_device && ssvh_bam_keep_names(src.bam, 1) != 0) die(string("[seeksv] ") + ssvh_last_error());
		ssv_batch_t b;
		while (src.next(&b, 1)) { // (every record's bases: the 3'-branch records without S are kept too)
			ssv_names_t nm;
			const int rc = src.on_device ? ssv_bamdec_names(ctx, &nm) : (ssvh_bam_batch_names(src.bam, &nm) == 0 ? SSV_OK : SSV_E_ARG);
			if (rc != SSV_OK) die(string("[seeksv] ") + (src.on_device ? ssv_last_error(ctx) : ssvh_last_error()));
			check(ctx, ssv_rt_scan(ctx, &b, &nm));
		}
		src.close();
	}
	ssv_rt_result res;
	check(ctx, ssv_rt_finish(ctx, &res));
	seeksv::apply_readthrough(res, names, junction2other);
}

// ---- N runs of records, one per GPU: every rank scans its own records for ALL junctions and windows; the partial tallies, depth sums
//      and point depths of the ranks meet in one all-gather (RCCL over xGMI between different GPUs) and are added up.  A rank replays
//      the records before its run through the pileup's read-cap bookkeeping first (ssv_getsv_prime). ----
// The one implementation behind `getsv -N`, `run -N` and `somatic -N`.  The callers differ in where a rank's records come from - its range of the file
// (`resident` empty), or the batches its context already holds, scanned in place - and in which vectors they want (n_counts / n_ranges / n_points == 0: not
// that one).  The replay's few thousand records are read from the file in either case.
struct RanksTally {
	string bam_path;
	const vector<ssvh_bam_part> *parts = nullptr;       // the cuts (ssvh_bam_partition), one per rank
	vector<ssv_ctx *> ctxs;                              // one per rank, the caller's
	vector<const vector<ssv_batch_t> *> resident;        // per rank: the retained batches of ITS context, in file order; empty: file ranges
	bool device_inflate = false;
	ssv_getsv_params gp;                                 // junctions, windows, thresholds, contig lengths
	bool depth = false;                                  // windows are scanned: a rank's pileup state is replayed
	const ssv_interval *ranges = nullptr, *points = nullptr;
	size_t n_counts = 0, n_ranges = 0, n_points = 0;
	int32_t *counts = nullptr; uint64_t *range_sum = nullptr; int32_t *point_depth = nullptr; // the ranks' sums are added to these
};

static void ranks_tally(const RanksTally &T)
{
	const int n_ranks = (int)T.ctxs.size();
	const string &original_bam = T.bam_path;
	const bool device_inflate = T.device_inflate, output_depth = T.depth;
	vector<ssv_ctx *> ctxs = T.ctxs;
	ssv_group *group = nullptr;
	if (ssv_group_create(ctxs.data(), n_ranks, &group) != SSV_OK) die(string("[seeksv] ") + ssv_last_error(nullptr));
	const size_t n_cnt = T.n_counts, n_rs = T.n_ranges, n_pd = T.n_points;
	const size_t vec_bytes = n_rs * 8 + (n_cnt + n_pd + 2) * 4; // [range sums u64 | counts i32 | point depths i32 | max depth, pad]
	vector<string> errs((size_t)n_ranks);
	vector<vector<uint8_t>> gathered((size_t)n_ranks);
	auto rank_main = [&](int r) {
		string &err = errs[(size_t)r];
		ssv_ctx *rc = ctxs[(size_t)r];
		const ssvh_bam_part &P = (*T.parts)[(size_t)r];
		const ssv_getsv_params &gp = T.gp;
		ssvh_bam *rb = nullptr;
		if (ssvh_bam_open(original_bam.c_str(), &rb) != 0) { err = "[main_samview] fail to open file for reading."; }
		// the pileup's state at the rank's first record: replay the records before it (more of them while the replay itself starts inside a
		// > 8000x stack; back to the file's first record at most)
		for (int64_t back = 24576; err.empty(); back *= 4) {
			if (ssv_getsv_begin(rc, &gp) != SSV_OK) { err = string("[seeksv] ") + ssv_last_error(rc); break; }
			if (r == 0 || !output_depth || P.own_coff == UINT64_MAX) break;
			uint64_t co; uint32_t uo; int64_t found = 0;
			if (ssvh_bam_walk_back(original_bam.c_str(), P.own_coff, P.own_uoff, back, &co, &uo, &found) != 0) { err = string("[seeksv] ") + ssvh_partition_last_error(); break; }
			if (found == 0) break;
			int32_t sufficient = 1;
			bool primed = false;
			if (device_inflate && found <= (1 << 22)) {
				// -Z: the replayed records are inflated and decoded on the rank's GPU like the run itself (one chunk: they are a few MB)
				BatchSource rs;
				rs.set_range(co, uo, P.own_coff, P.own_uoff);
				rs.open(original_bam, rc, true, "[main_samview] fail to open file for reading.");
				ssv_batch_t db, more;
				if (rs.next(&db, 0)) {
					if (ssv_getsv_prime(rc, &db, &sufficient) != SSV_OK) { err = string("[seeksv] ") + ssv_last_error(rc); rs.close(); break; }
					primed = !rs.next(&more, 0); // (a replay that spans chunks goes through the host reader below: the bookkeeping takes one batch)
				}
				rs.close();
				if (!primed && ssv_getsv_begin(rc, &gp) != SSV_OK) { err = string("[seeksv] ") + ssv_last_error(rc); break; }
			}
			if (!primed) {
				if (ssvh_bam_set_range(rb, co, uo, P.own_coff, P.own_uoff) != 0) { err = string("[seeksv] ") + ssvh_last_error(); break; }
				ssv_batch_t hb;
				if (ssvh_bam_read_batch(rb, found + 16, 0, &hb) != 0) { err = string("[seeksv] ") + ssvh_last_error(); break; }
				if (ssv_getsv_prime(rc, &hb, &sufficient) != SSV_OK) { err = string("[seeksv] ") + ssv_last_error(rc); break; }
			}
			if (sufficient || found < back) break; // (found < back: the replay began at the file's first record - as far back as a replay can start)
		}
		auto scan = [&](const ssv_batch_t &b) { if (err.empty() && ssv_getsv_scan(rc, &b) != SSV_OK) err = string("[seeksv] ") + ssv_last_error(rc); };
		if (err.empty() && !T.resident.empty()) { // the run itself: where the rank's getclip left it, in this context's memory
			for (const ssv_batch_t &b : *T.resident[(size_t)r]) scan(b);
		} else if (err.empty()) { // the run itself: host threads or the GPU (-Z) inflate and decode its blocks
			BatchSource src;
			src.set_range(P.own_coff, P.own_uoff, P.end_coff, P.end_uoff);
			src.open(original_bam, rc, device_inflate, "[main_samview] fail to open file for reading.");
			src.pump(0, [](const ssv_batch_t &) {}, scan);
			src.close();
		}
		vector<uint8_t> mine(vec_bytes, 0);
		uint64_t *v_rs = reinterpret_cast<uint64_t *>(mine.data());
		int32_t *v_cnt = reinterpret_cast<int32_t *>(mine.data() + n_rs * 8), *v_pd = v_cnt + n_cnt, *v_max = v_pd + n_pd;
		vector<int32_t> tmp_cnt(n_cnt + 1), tmp_pd(n_pd + 1);
		vector<uint64_t> tmp_rs(n_rs + 1);
		if (err.empty() && ssv_getsv_finish(rc, T.counts ? tmp_cnt.data() : nullptr, T.ranges, (int64_t)n_rs, tmp_rs.data(), T.points, (int64_t)n_pd, tmp_pd.data(), v_max) != SSV_OK)
			err = string("[seeksv] ") + ssv_last_error(rc);
		if (n_rs) memcpy(v_rs, tmp_rs.data(), n_rs * 8);
		if (n_cnt) memcpy(v_cnt, tmp_cnt.data(), n_cnt * 4);
		if (n_pd) memcpy(v_pd, tmp_pd.data(), n_pd * 4);
		// the exchange: every rank takes part, also one that failed (its vector is zero; the error is reported afterwards)
		gathered[(size_t)r].assign(vec_bytes * (size_t)n_ranks, 0);
		if (ssv_group_allgather(group, r, mine.data(), vec_bytes, gathered[(size_t)r].data()) != SSV_OK && err.empty()) err = string("[seeksv] ") + ssv_last_error(rc);
		if (rb) ssvh_bam_close(rb);
	};
	{
		vector<std::thread> th;
		for (int r = 1; r < n_ranks; ++r) th.emplace_back(rank_main, r);
		rank_main(0);
		for (auto &x : th) x.join();
	}
	for (auto &e : errs) if (!e.empty()) die(e);
	// rank 0's copy of the gathered vectors: the sums are the whole file's tallies and depths
	for (int r = 0; r < n_ranks; ++r) {
		const uint8_t *v = gathered[0].data() + (size_t)r * vec_bytes;
		const uint64_t *v_rs = reinterpret_cast<const uint64_t *>(v);
		const int32_t *v_cnt = reinterpret_cast<const int32_t *>(v + n_rs * 8), *v_pd = v_cnt + n_cnt;
		for (size_t k = 0; k < n_rs; ++k) T.range_sum[k] += v_rs[k];
		for (size_t k = 0; k < n_cnt; ++k) T.counts[k] += v_cnt[k];
		for (size_t k = 0; k < n_pd; ++k) T.point_depth[k] += v_pd[k];
	}
	if (getenv("SSV_TIMING")) cerr << "[timing] exchange over " << (ssv_group_uses_rccl(group) ? "RCCL (ncclAllGather)" : "host memory (ranks share a GPU)") << ", " << vec_bytes << " bytes per rank" << endl;
	ssv_group_destroy(group);
}

// One tally over a BAM for getsv and somatic: T holds the filled ssv_getsv_params, what to sum and where to.  n_ranks == 0, one GPU: begin, scan - the insert-size
// pass's carry (its kept batches, then what its open source still holds) or a fresh source over the file, which under `seeksv run` is the batches the session's context
// holds -, finish.  n_ranks >= 1: ranks_tally over a session's ranks where they lie (its cuts, contexts and batches), else over file ranges cut here, contexts 1..n-1 made here.
static void tally_records(ssv_ctx *ctx, RanksTally &T, int n_ranks, const vector<int> &devices, IsizeCarry &carry, const RunSession *run)
{
	if (n_ranks) {
		const RunRanks *const ranks = run && run->ranked() ? &run->ranks : nullptr;
		vector<ssvh_bam_part> parts((size_t)n_ranks);
		if (!ranks && ssvh_bam_partition(T.bam_path.c_str(), n_ranks, 0, parts.data()) != 0) die(string("[seeksv] ") + ssvh_partition_last_error());
		T.parts = ranks ? &ranks->parts : &parts;
		T.ctxs.assign((size_t)n_ranks, nullptr);
		T.ctxs[0] = ctx;
		for (int r = 1; r < n_ranks; ++r) {
			if (ranks) T.ctxs[(size_t)r] = ranks->rank[(size_t)r].ctx;
			else if (ssv_ctx_create(device_of_rank(r, devices), &T.ctxs[(size_t)r]) != SSV_OK) die(string("[seeksv] ") + ssv_last_error(nullptr));
		}
		if (ranks) for (const RunRank &k : ranks->rank) T.resident.push_back(&k.batches);
		ranks_tally(T);
		if (!ranks) for (int r = 1; r < n_ranks; ++r) ssv_ctx_destroy(T.ctxs[(size_t)r]);
	} else {
		check(ctx, ssv_getsv_begin(ctx, &T.gp));
		auto scan = [&](const ssv_batch_t &b) { check(ctx, ssv_getsv_scan(ctx, &b)); };
		if (carry.usable) { // the insert-size pass left its source open behind the chunks it read, whose batches are still valid: ONE reading of the file
			for (auto &k : carry.kept) scan(k);
			carry.src.pump(0, [](const ssv_batch_t &) {}, scan);
		} else {
			BatchSource src; // a second handle: the caller's keeps serving the header
			src.open(T.bam_path, [ctx] { return ctx; }, T.device_inflate, "[main_samview] fail to open file for reading.", run);
			src.pump(0, [](const ssv_batch_t &) {}, scan);
			src.close();
		}
		int32_t maxd = 0;
		check(ctx, ssv_getsv_finish(ctx, T.counts, T.ranges, (int64_t)T.n_ranges, T.range_sum, T.points, (int64_t)T.n_points, T.point_depth, &maxd));
	}
	carry.drop(ctx);
}

struct GetsvOptions {
	string connect_bam, temp_breakpoint, dump_junctions; // -F, -B, -J: empty = not given
	double frequency = 0.1;
	int min_mapQ2 = 1, min_mapQ = 20, read_pair_used = 5000000, sum_min_no_both_clipped_reads = 3, min_distance = 50, microhomology_length = 50, device = 0,
	    min_abnormal_read_pair_no = 0, flank_length = 200, min_seq_len = 30, max_seq_indel_no = 1, flank = 50, n_ranks = 1;
	bool output_depth = true, device_inflate = device_inflate_default(), verify_crc = false, ranks_given = false, devices_given = false;
	vector<int> devices;
	string clip_bam, original_bam, clipfile, breakpoint_file, clip_unmap_fq_file;
	void set_devices(const char *list) { devices = parse_devices(list); device = devices.empty() ? 0 : devices[0]; }
};

static GetsvOptions parse_getsv(int argc, char **argv, bool for_run = false)
{
	GetsvOptions o;
	int c;
	optind = 0;
	while ((c = getopt(argc, argv, "F:B:t:l:q:Q:w:n:a:b:d:e:m:i:R:f:T:L:rDG:J:ZCN:")) >= 0) {
		switch (c) {
		case 'F': o.connect_bam = optarg; break;
		case 'B': o.temp_breakpoint = optarg; break;
		case 'l': o.flank = atoi(optarg); break;
		case 'q': o.min_mapQ = atoi(optarg); break;
		case 'n': o.read_pair_used = atoi(optarg); break;
		case 'b': o.sum_min_no_both_clipped_reads = atoi(optarg); break;
		case 'd': o.min_distance = atoi(optarg); break;
		case 'e': o.min_abnormal_read_pair_no = atoi(optarg); break;
		case 'm': o.min_seq_len = atoi(optarg); break;
		case 'i': o.max_seq_indel_no = atoi(optarg); break;
		case 'D': o.output_depth = false; break;
		case 'f': o.frequency = atof(optarg); break;
		case 'T': o.microhomology_length = atoi(optarg); break;
		case 'L': o.flank_length = atoi(optarg); break;
		case 'G': o.set_devices(optarg); o.devices_given = true; break;
		case 'Z': o.device_inflate = true; break;
		case 'C': o.verify_crc = true; break;
		case 'N': o.n_ranks = atoi(optarg); o.ranks_given = true; break;
		case 'J': o.dump_junctions = optarg; break;
		case 'w': o.min_mapQ2 = atoi(optarg); break; // -F's mapping-quality floor (seeksv.cpp:221-225)
		default: break; // -t -Q -a -R -r: accepted, unused (as in the reference, where -t / -Q no longer reach the join)
		}
	}
	if (argc != optind + (for_run ? 0 : 5)) usage_getsv();
	if (o.flank > 90 || o.flank < 0 || o.min_seq_len < 0 || o.n_ranks < 1) usage_getsv();
	if (!for_run) { o.clip_bam = argv[optind]; o.original_bam = argv[optind + 1]; o.clipfile = argv[optind + 2]; o.breakpoint_file = argv[optind + 3]; o.clip_unmap_fq_file = argv[optind + 4]; }
	return o;
}

static int getsv_main(const GetsvOptions &opt, RunSession *run)
{
	PhaseTimer pt;
	if (opt.verify_crc) g_verify_crc = true;
	const int times = 4;
	double frequency = opt.frequency;
	int min_abnormal_read_pair_no = opt.min_abnormal_read_pair_no;
	JunctionMap junction2other;
	if (!opt.temp_breakpoint.empty()) { // ReadBreakpoint, getsv.cpp:1292-1323
		ifstream fin(opt.temp_breakpoint.c_str());
		if (!fin) cerr << "Cannot open file " << opt.temp_breakpoint << endl;
		string up_chr, down_chr, svt, up_cigar, down_cigar, up_seq, down_seq, temp;
		int up_pos, up_reads_no, down_pos, down_reads_no, micro, abnormal, d1, d2, d3, d4, d5, d6;
		char up_strand, down_strand;
		double r1, r2;
		while (fin >> up_chr) {
			if (up_chr[0] == '@') { getline(fin, temp); continue; }
			fin >> up_pos >> up_strand >> up_reads_no >> down_chr >> down_pos >> down_strand >> down_reads_no >> micro >> abnormal >> svt >> d1 >> d2 >> d3 >> d4 >> d5 >> d6 >> r1 >> r2 >>
			    up_cigar >> down_cigar >> up_seq >> down_seq;
			getline(fin, temp);
			Junction j{up_chr, up_pos, up_strand, down_chr, down_pos, down_strand};
			OtherInfo o;
			o.up.seq = up_seq; o.up.cigar_vec = parse_cigar(up_cigar); o.up.support = up_reads_no;
			o.down.seq = down_seq; o.down.cigar_vec = parse_cigar(down_cigar); o.down.support = down_reads_no;
			o.microhomology = micro; o.abnormal = abnormal;
			junction2other.insert(make_pair(j, o));
		}
		cerr << "[ReadBreakpoint] finish" << endl;
	}
	ssv_ctx *rt_ctx = nullptr;
	if (!opt.connect_bam.empty()) { // FindJunction (seeksv.cpp:221-225): after the -B rows, before the clip join; with -N n once, on the first device
		rt_ctx = acquire_ctx(opt.device, run);
		readthrough_pass(opt.connect_bam, opt.min_mapQ2, rt_ctx, opt.device_inflate, junction2other);
		cerr << "'FindJunction' finished" << endl;
		pt.lap("readthrough (-F)");
	} else if (run && run->split_leg) { // `seeksv run -P`: at the same place, with -w as its floor
		rt_ctx = acquire_ctx(opt.device, run);
		run->split_leg(rt_ctx, opt.min_mapQ2, junction2other);
		cerr << "'FindJunction' finished" << endl;
		pt.lap("readthrough (run -P: split alignments of the unmapped pairs, device rows)");
	} else if (run && run->splitread_open) { // `seeksv run -A`: at the same place; the session has seen every chunk of the original
		rt_ctx = acquire_ctx(opt.device, run);
		if (pt.on) { ssv_prof_enable(rt_ctx, 1); ssv_prof_reset(rt_ctx); }
		ssv_rt_result res;
		check(rt_ctx, ssv_rt_finish(rt_ctx, &res));
		run->splitread_open = false;
		seeksv::apply_readthrough(res, run->splitread_names, junction2other);
		ssv_rt_original_counts st;
		check(rt_ctx, ssv_rt_original_stats(rt_ctx, &st));
		cerr << "[seeksv] -A: " << st.pairs << " pairs (" << st.pairs_borrowed << " with a borrowed seq) of " << st.candidates << " one-side-clipped records (" << st.hard_clipped
		     << " hard-clipped); dropped at the pairing: " << st.dropped_no_carrier << " without a record that carries the read, " << st.dropped_length << " for unequal read lengths" << endl;
		if (run->splitread_sa) {
			ssv_rt_original_sa_counts sa;
			check(rt_ctx, ssv_rt_original_sa_stats(rt_ctx, &sa));
			cerr << "[seeksv] -S: sa_tags " << sa.sa_tags << ", sa_multi " << sa.sa_multi << ", sa_refused " << sa.sa_refused << ", virtuals " << sa.virtuals << ", sa_redundant " << sa.sa_redundant
			     << ", pairs_from_sa " << sa.pairs_from_sa << ", sa_dropped_length " << sa.sa_dropped_length << endl;
		}
		pt.lap("splitread (run -A: the original's own supplementary alignments)");
		if (pt.on && run->splitread_sa) {
			double ms = 0; int64_t launches = 0;
			ssv_prof_get(rt_ctx, "splitread_sa_finish", &ms, &launches, nullptr);
			cerr << "[timing] (-A -S kernel time: splitread_sa_aux " << run->splitread_aux_ms << " ms in " << run->splitread_aux_launches << " launches, splitread_sa_scan " << run->splitread_scan_ms << " ms in "
			     << run->splitread_scan_launches << " launches, splitread_sa_finish " << ms << " ms in " << launches << " launches; the scans held the pump for " << run->splitread_scan_wall
			     << " s; candidate store " << st.store_bytes << " bytes)" << endl;
			ssv_prof_enable(rt_ctx, 0);
		} else if (pt.on) {
			double ms = 0; int64_t launches = 0;
			ssv_prof_get(rt_ctx, "splitread_finish", &ms, &launches, nullptr);
			cerr << "[timing] (-A kernel time: splitread_scan " << run->splitread_scan_ms << " ms in " << run->splitread_scan_launches << " launches, splitread_finish " << ms << " ms in " << launches
			     << " launches; the scans held the pump for " << run->splitread_scan_wall << " s; candidate store " << st.store_bytes << " bytes)" << endl;
			ssv_prof_enable(rt_ctx, 0);
		}
	}
	{ // InputSoftInfoStoreBreakpoint + GetJunction (getsv.h:423, getsv.cpp:1705): clip clusters x re-alignments of their clipped sequences
		string err;
		const bool rows_resident = run && run->rows_kept; // the rows of prefix.clip.gz are still in memory
		auto join_records = [&](const seeksv::AlnRecords &R) { // the alignments in memory; the rows too when this process wrote them
			if (!rows_resident) return seeksv::assemble_junctions_file_records(opt.clipfile, R, junction2other);
			if (run->all_clean() && !getenv("SSV_RUN_PARSE_ROWS")) { // the rows as the formatter kept them: nothing is parsed (SSV_RUN_PARSE_ROWS, tests: the text is)
				vector<const vector<seeksv::ClipRow> *> parts;
				for (const auto &p : run->pieces) parts.push_back(&p.parsed);
				return seeksv::assemble_junctions_rows(parts, R, junction2other);
			}
			return seeksv::assemble_junctions_records(run->row_views(), R, junction2other);
		};
		if (!is_bam_name(opt.clip_bam)) { // SAM text (the reference's rule, getsv.h:437-446): always parsed on the GPU, whatever -Z says; with -N n once, on the first device
			if (!rt_ctx) { rt_ctx = acquire_ctx(opt.device, run); pt.lap("context start-up (waited for in front of the SAM decode)"); }
			ClipAlignments A;
			clip_sam_pass(opt.clip_bam, rt_ctx, A);
			pt.lap("clip alignments (SAM text: decode + pack)");
			err = join_records(A.R);
		} else if (rows_resident && run->aln.rec) {
			seeksv::AlnRecords R; // rows and alignments are both still in memory
			resident_alignments(*run, R);
			err = join_records(R);
		} else err = rows_resident ? seeksv::assemble_junctions_text(run->row_views(), opt.clip_bam, junction2other) : seeksv::assemble_junctions(opt.clipfile, opt.clip_bam, junction2other);
		if (!err.empty()) die(err);
	}
	cerr << "'InputSoftInfoStoreBreakpoint' finished" << endl;
	seeksv::merge_junctions(junction2other, opt.flank); // MergeJunction(flank = -l)
	if (!opt.dump_junctions.empty()) { // test hook: the junction table before any BAM pass (no GPU needed)
		ofstream jd(opt.dump_junctions.c_str());
		for (auto &kv : junction2other) {
			const Junction &j = kv.first; const OtherInfo &o = kv.second;
			jd << j.up_chr << '\t' << j.up_pos << '\t' << j.up_strand << '\t' << o.up.support << '\t' << j.down_chr << '\t' << j.down_pos << '\t' << j.down_strand << '\t' << o.down.support << '\t'
			   << o.microhomology << '\t' << o.abnormal << '\t' << sv_type(j) << "\t0\t0\t0\t0\t0\t0\t0\t0\t" << cigar_text(o.up) << '\t' << cigar_text(o.down) << '\t' << o.up.seq << '\t' << o.down.seq
			   << '\t' << o.up.uniq << '\t' << o.down.uniq << '\n';
		}
		return 0;
	}

	pt.lap("junction_stage");
	ssvh_bam *bam = nullptr;
	if (run && run->text_input) { // `seeksv run` on SAM text: the header getclip read (the text itself is gone, its records are in HBM)
		bam = text_header_handle(run->text_names, run->text_lens);
	} else if (ssvh_bam_open(opt.original_bam.c_str(), &bam) != 0) die("[main_samview] fail to open file " + opt.original_bam + "for reading.");
	ssv_ctx *ctx = rt_ctx;
	auto get_ctx = [&] { if (!ctx) ctx = acquire_ctx(opt.device, run); return ctx; }; // (main() started it before the junction stage)

	int mean_insert_size = 0, deviation = 0;
	const bool do_discordant = opt.read_pair_used >= 100000; // seeksv.cpp:246
	IsizeCarry carry;
	// SSV_GROUP_RCCL_ONE=1: `-N 1` takes the ranks' path too - one run of records, its vector through a one-rank RCCL communicator (what a
	// one-GPU box can execute of the exchange)
	const bool ranks_path = opt.n_ranks > 1 || getenv("SSV_GROUP_RCCL_ONE");
	if (do_discordant) {
		insert_size_pass(get_ctx, opt.original_bam, opt.device_inflate, opt.min_mapQ, opt.read_pair_used, mean_insert_size, deviation, !ranks_path ? &carry : nullptr, run);
		cerr << "'CalculateInsertsizeDeviation' finished" << endl;
	} else min_abnormal_read_pair_no = 0; // seeksv.cpp:285
	get_ctx();

	pt.lap("isize_pass (+ what was left of the context's start-up)");
	// ---- the fused BAM pass: discordant tally + depth ----
	vector<ssvh_junction_in> J;
	vector<int32_t> prev;
	for (auto &kv : junction2other) {
		J.push_back(ssvh_junction_in{kv.first.up_chr.c_str(), kv.first.down_chr.c_str(), kv.first.up_pos, kv.first.down_pos, kv.first.up_strand, kv.first.down_strand});
		prev.push_back(kv.second.abnormal);
	}
	const int64_t nJ = (int64_t)J.size();
	ssvh_plan *plan = nullptr;
	ssvh_plan_create(bam, J.data(), nJ, nullptr, nullptr, 0, mean_insert_size, deviation, times, opt.flank_length, &plan);
	int64_t nj, nw, nr, np;
	const ssv_junction *dj = ssvh_plan_junctions(plan, &nj);
	const ssv_interval *dw = ssvh_plan_windows(plan, &nw);
	const ssv_interval *dr = ssvh_plan_ranges(plan, &nr);
	const ssv_interval *dp = ssvh_plan_points(plan, &np);
	pt.lap("plan");
	vector<int32_t> counts((size_t)nj + 1, 0), pdepth((size_t)np + 1, 0);
	vector<uint64_t> rsum((size_t)nr + 1, 0);
	if (do_discordant || opt.output_depth) {
		// `seeksv run -N`: the cuts getclip's ranks used, their contexts, and the records where those ranks left them; else the file is cut here and read
		RanksTally T;
		T.bam_path = opt.original_bam; T.device_inflate = opt.device_inflate;
		memset(&T.gp, 0, sizeof(T.gp));
		T.gp.junctions = dj; T.gp.n_junctions = do_discordant ? nj : 0;
		T.gp.mean = mean_insert_size; T.gp.sd = deviation; T.gp.times = times; T.gp.disc_min_mapq = opt.min_mapQ;
		T.gp.windows = dw; T.gp.n_windows = opt.output_depth ? nw : 0; T.gp.depth_min_mapq = opt.min_mapQ;
		T.gp.n_targets = ssvh_bam_n_targets(bam); T.gp.target_len = ssvh_bam_target_lens(bam);
		T.depth = opt.output_depth;
		T.ranges = dr; T.points = dp;
		T.n_counts = do_discordant ? (size_t)nj : 0; T.n_ranges = opt.output_depth ? (size_t)nr : 0; T.n_points = opt.output_depth ? (size_t)np : 0;
		T.counts = do_discordant ? counts.data() : nullptr; T.range_sum = rsum.data(); T.point_depth = pdepth.data();
		tally_records(ctx, T, ranks_path ? opt.n_ranks : 0, opt.devices, carry, run);
	}
	pt.lap("fused_pass");
	if (do_discordant) { cerr << "'StoreSeqName2Tid' finished" << endl; cerr << "'FindDiscordantReadPairs' finished" << endl; }
	if (opt.output_depth) { cerr << "'MergeOverlap' finished" << endl; cerr << "'main_depth' finished" << endl; }
	else frequency = 0; // seeksv.cpp:300
	vector<int32_t> abnormal((size_t)nJ + 1), up_depth((size_t)nJ + 1), down_depth((size_t)nJ + 1);
	vector<uint64_t> flank_sum((size_t)nJ * 4 + 4);
	vector<uint32_t> flank_len((size_t)nJ * 4 + 4);
	ssvh_plan_fold(plan, do_discordant ? counts.data() : nullptr, prev.data(), rsum.data(), pdepth.data(), abnormal.data(), up_depth.data(), down_depth.data(), flank_sum.data(),
	               flank_len.data(), nullptr);

	ofstream fout(opt.breakpoint_file.c_str());
	if (!fout) die("Cannot open file " + opt.breakpoint_file);
	fout << "@left_chr\tleft_pos\tleft_strand\tleft_clip_read_NO\tright_chr\tright_pos\tright_strand\tright_clip_read_NO\tmicrohomology_length\tabnormal_readpair_NO\tsvtype\tleft_pos_depth\t"
	        "right_pos_depth\taverage_depth_of_left_pos_5end\taverage_depth_of_left_pos_3end\taverage_depth_of_right_pos_5end\taverage_depth_of_right_pos_3end\tleft_pos_clip_percentage\t"
	        "right_pos_clip_percentage\tleft_seq_cigar\tright_seq_cigar\tleft_seq\tright_seq" << endl;
	// OutputBreakpoint, getsv.cpp:838-987
	int64_t idx = 0;
	for (auto it = junction2other.begin(); it != junction2other.end(); ++it, ++idx) {
		const Junction &j = it->first;
		OtherInfo &o = it->second;
		if (do_discordant) o.abnormal = abnormal[(size_t)idx];
		const int updepth = (opt.output_depth ? up_depth[(size_t)idx] : 0) + o.down.support;     // without the depth pass pos2depth is empty: the reference prints an error and uses 0
		const int downdepth = (opt.output_depth ? down_depth[(size_t)idx] : 0) + o.up.support;
		const int up_only = opt.output_depth ? updepth : 0, down_only = opt.output_depth ? downdepth : 0;
		if (!opt.output_depth) {
			cerr << "Error: There is something wrong in upstream position " << j.up_chr << ":" << j.up_pos << endl;
			cerr << "Error: There is something wrong in downstream position " << j.down_chr << ":" << j.down_pos << endl;
		}
		const int ud = up_only, dd = down_only;
		const int junction_reads_no = o.up.support + o.down.support;
		const double rate1 = ud == 0 ? 0 : (double)junction_reads_no / ud, rate2 = dd == 0 ? 0 : (double)junction_reads_no / dd;
		auto filtered = [&](const char *reason) { // OutputFilteredBreakpoint, getsv.cpp:1846
			cout << reason << '\t' << j.up_chr << '\t' << j.up_pos << '\t' << j.up_strand << '\t' << o.up.support << '\t' << j.down_chr << '\t' << j.down_pos << '\t' << j.down_strand << '\t'
			     << o.down.support << '\t' << o.microhomology << '\t' << o.abnormal << '\t' << sv_type(j) << '\t' << ud << '\t' << dd << '\t' << rate1 << '\t' << rate2 << '\t'
			     << cigar_text(o.up) << '\t' << cigar_text(o.down) << '\t' << o.up.seq << '\t' << o.down.seq << endl;
		};
		if (!(o.up.uniq + o.down.uniq >= 2 || o.abnormal > 0)) { filtered("mappingQ_too_low"); continue; }
		if (j.up_chr == j.down_chr && abs(j.up_pos - j.down_pos) < opt.min_distance) { filtered("distance_too_near"); continue; }
		if (o.microhomology > opt.microhomology_length) { filtered("microhomology_len_too_long"); continue; }
		if (o.abnormal < min_abnormal_read_pair_no) { filtered("abnormal_read_pair_no_not_pass"); continue; }
		if ((o.up.support > 0 && o.down.support > 0 && rate1 < frequency && rate2 < frequency) || (o.up.support == 0 && rate2 < frequency) || (o.down.support == 0 && rate1 < frequency)) {
			filtered("frequency_too_low"); continue;
		}
		if (o.up.support + o.down.support < opt.sum_min_no_both_clipped_reads) { filtered("total_clipped_reads_NO_not_pass"); continue; }
		if (o.abnormal == 0) {
			if (o.up.seq.length() < (size_t)(o.up.left_clipped + o.up.right_clipped + opt.min_seq_len) || o.down.seq.length() < (size_t)(o.down.left_clipped + o.down.right_clipped + opt.min_seq_len)) {
				filtered("seq_length_too_short"); continue;
			}
			if (o.up.cigar_vec.size() > (size_t)(2 * opt.max_seq_indel_no + 1) || o.down.cigar_vec.size() > (size_t)(2 * opt.max_seq_indel_no + 1)) { filtered("seq_with_too_many_indels"); continue; }
			if (largest_base_frequency(o.up.seq) >= 0.8 || largest_base_frequency(o.down.seq) >= 0.8) { filtered("repeat_bases"); continue; }
		}
		unsigned int fl[4] = {0, 0, 0, 0};
		if (opt.output_depth) for (int k = 0; k < 4; ++k) fl[k] = (unsigned int)(flank_sum[(size_t)idx * 4 + k] / flank_len[(size_t)idx * 4 + k]); // getsv.cpp:946 (divides by zero like the reference if a window is empty)
		else cerr << "Error depth in the vicinity of junction " << j.up_chr << '\t' << j.up_pos << '\t' << j.up_strand << '\t' << j.down_chr << '\t' << j.down_pos << '\t' << j.down_strand << endl;
		fout << j.up_chr << '\t' << j.up_pos << '\t' << j.up_strand << '\t' << o.up.support << '\t' << j.down_chr << '\t' << j.down_pos << '\t' << j.down_strand << '\t' << o.down.support << '\t'
		     << o.microhomology << '\t' << o.abnormal << '\t' << sv_type(j) << '\t' << ud << '\t' << dd << '\t' << (int)fl[0] << '\t' << (int)fl[1] << '\t' << (int)fl[2] << '\t' << (int)fl[3] << '\t'
		     << rate1 << '\t' << rate2 << '\t' << cigar_text(o.up) << '\t' << cigar_text(o.down) << '\t' << o.up.seq << '\t' << o.down.seq << endl;
	}
	ofstream foutuq(opt.clip_unmap_fq_file.c_str()); // OutputOneendUnmapBreakpoint: always empty (GetJunction returns early for type 'n')
	if (!foutuq) die("Cannot open file " + opt.clip_unmap_fq_file);
	pt.lap("fold+output");
	ssvh_plan_destroy(plan);
	release_ctx(ctx, run);
	ssvh_bam_close(bam);
	pt.lap("teardown");
	return 0;
}


static int cmd_getsv(int argc, char **argv) { return getsv_main(parse_getsv(argc, argv), nullptr); }

// ---------------------------------------------------------------------------------------------------------------------
// somatic (CallSomatic, seeksv.cpp:366-407; ReadTumorFileAndOutputSomaticInfo, somatic.cpp:14-427)
// ---------------------------------------------------------------------------------------------------------------------

static vector<string> split_words(const string &t)
{
	vector<string> w;
	std::istringstream in(t);
	for (string x; in >> x;) w.push_back(x);
	return w;
}

// the words of run's -c / -v / -a through the step's own parser (words[0]: the step's name, as getopt prints it)
template <class Options> static Options parse_words(const char *step, const string &text, Options (*parse)(int, char **, bool))
{
	vector<string> words = {step};
	for (auto &x : split_words(text)) words.push_back(x);
	vector<char *> av;
	for (auto &w : words) av.push_back(const_cast<char *>(w.c_str()));
	av.push_back(nullptr);
	return parse((int)words.size(), av.data(), true);
}

struct SomaticOptions {
	int offset = 30, min_len_of_clipped_seq = 10, read_pair_used = 5000000, min_mapQ = 20, device = 0, n_ranks = 1;
	double min_map_rate = 0.9;
	string dump_lookups; // -J
	bool device_inflate = device_inflate_default(), verify_crc = false;
	vector<int> devices;
	string normal_bam_file, clipped_file, tumor_file, somatic_file;
	bool mark_dups = false; // -M (with -K): duplicate read pairs of the normal are marked where its records are retained
	bool pair_dups = false; // -D (with -K): ... by the unclipped 5' ends of both reads, once all its records are retained
	string include_file, exclude_file; // -L / -X (with -K): the normal's retained records are restricted to a BED file's regions
	bool from_bam = false; // -K: no clip.gz - the normal's clusters come from its BAM, and the look-ups run on the GPU where the clusters lie
	GetclipOptions clip;   // -K: the clip pass's options (-c: getclip's -t / -q / -s; the defaults are getclip's)
};

static SomaticOptions parse_somatic(int argc, char **argv)
{
	SomaticOptions o;
	int c;
	optind = 0;
	string clip_opts;
	bool clip_opts_given = false;
	while ((c = getopt(argc, argv, "t:q:l:m:n:G:J:ZCN:Kc:MDL:X:")) >= 0) {
		switch (c) {
		case 't': o.min_map_rate = atof(optarg); break;
		case 'q': o.min_mapQ = atoi(optarg); break;
		case 'l': o.offset = atoi(optarg); break;
		case 'm': o.min_len_of_clipped_seq = atoi(optarg); break;
		case 'n': o.read_pair_used = atoi(optarg); break;
		case 'G': o.devices = parse_devices(optarg); o.device = o.devices.empty() ? 0 : o.devices[0]; break;
		case 'Z': o.device_inflate = true; break;
		case 'C': o.verify_crc = true; break;
		case 'N': o.n_ranks = atoi(optarg); break;
		case 'J': o.dump_lookups = optarg; break; // test hook: the look-ups only (no insert-size or tally pass; without -K no BAM pass and no GPU), one line per output row
		case 'K': o.from_bam = true; break;
		case 'M': o.mark_dups = true; break;
		case 'D': o.pair_dups = true; break;
		case 'L': o.include_file = optarg; break;
		case 'X': o.exclude_file = optarg; break;
		case 'c': clip_opts = optarg; clip_opts_given = true; break;
		}
	}
	if (o.n_ranks < 1) usage_somatic();
	if (o.mark_dups && !o.from_bam) die("seeksv somatic: -M marks duplicates where the clip pass of -K retains the normal's records; without -K there is no such pass");
	if (o.pair_dups && !o.from_bam) die("seeksv somatic: -D marks duplicate pairs once the clip pass of -K has retained the normal's records; without -K there is no such pass");
	if (o.pair_dups && o.mark_dups) die("seeksv somatic: -D and -M are two rules for the one duplicate flag; -M is not supported with -D");
	if ((!o.include_file.empty() || !o.exclude_file.empty()) && !o.from_bam)
		die("seeksv somatic: -L and -X restrict the records that the clip pass of -K retains; without -K there is no such pass");
	if (!o.include_file.empty() && !o.exclude_file.empty()) die("seeksv somatic: -L keeps the records inside its regions and -X those outside; -X is not supported with -L");
	if (clip_opts_given && !o.from_bam) die("seeksv somatic: -c hands getclip's options to the clip pass of -K; without -K there is no such pass");
	if (argc != optind + (o.from_bam ? 3 : 4)) { cerr << argc << '\t' << optind << endl; usage_somatic(); }
	else if (o.offset >= 90 || o.offset < 0) { cerr << "Error: value of -l must in range [0, 90) " << endl; usage_somatic(); }
	o.normal_bam_file = argv[optind];
	if (!o.from_bam) { o.clipped_file = argv[optind + 1]; o.tumor_file = argv[optind + 2]; o.somatic_file = argv[optind + 3]; return o; }
	o.tumor_file = argv[optind + 1]; o.somatic_file = argv[optind + 2];
	// -K: refused before anything is written
	o.clip = parse_words("getclip", clip_opts, parse_getclip);
	if (o.clip.ranks_given || o.clip.devices_given || o.clip.prefix_given)
		die("seeksv somatic -K: -N, -G or -o inside -c is not supported; the clip pass runs on somatic's own GPU (-G) and writes no file");
	if (o.n_ranks > 1) die("seeksv somatic -K: -N above 1 is not supported; the look-ups run against one GPU's cluster tables");
	if (!is_bam_name(o.normal_bam_file)) die("seeksv somatic -K: the normal must be a BAM (a name ending in .bam); SAM text is not supported");
	o.clip.bamfile = o.normal_bam_file; o.clip.device = o.device; o.clip.devices = vector<int>(1, o.device); o.clip.n_ranks = 1;
	o.clip.device_inflate = true; // (as `seeksv run`: decoded on the GPU, where the records stay)
	o.clip.mark_dups = o.mark_dups; o.clip.pair_dups = o.pair_dups;
	o.clip.regions_file = o.include_file.empty() ? o.exclude_file : o.include_file; o.clip.regions_exclude = o.include_file.empty() && !o.exclude_file.empty();
	if (o.verify_crc) o.clip.verify_crc = true;
	return o;
}

static void dump_lookups(const string &path, const vector<SomaticRow> &rows)
{
	ofstream jd(path.c_str());
	for (auto &row : rows) {
		if (row.kind == SomaticRow::HEADER) jd << row.text << '\n';
		else if (row.kind == SomaticRow::MESSAGE) cerr << row.text << endl;
		else jd << row.text << '\t' << row.normal_left_reads << '\t' << row.normal_right_reads << '\n';
	}
}

// `somatic -K`, first half: the tumor rows' look-ups as probes (build_cluster_probes), set in the library, and ONE getclip pass over the normal BAM through the session
// machinery of `seeksv run` - its batches stay in HBM for the insert-size and tally passes, every pass's cluster table is probed on the GPU where it lies
// (ssv_clip_cluster with probes set), nothing is written.  rows: the table's rows with both look-ups done.  Returns the session that holds the records.
static RunSession *somatic_clip_pass(const SomaticOptions &o, vector<SomaticRow> &rows, PhaseTimer &pt)
{
	ssvh_bam *bam = nullptr;
	if (ssvh_bam_open(o.normal_bam_file.c_str(), &bam) != 0) die("[main_samview] fail to open file for reading.");
	{
		const string err = parse_tumor_table(o.tumor_file, 1, rows); // (what a row asks of the clusters does not depend on the insert size; `tally` is set by the caller's own parse)
		if (!err.empty()) die(err);
	}
	vector<seeksv::ClusterProbe> probes;
	vector<pair<int, int>> of_row;
	seeksv::build_cluster_probes(rows, o.offset, probes, of_row);
	std::unordered_map<string, int32_t> tid_of; // contig names to ids by the normal's header (the first of equal names)
	for (int32_t t = 0, nt = ssvh_bam_n_targets(bam); t < nt; ++t) { const char *nm = ssvh_bam_target_name(bam, t); tid_of.emplace(nm ? nm : "", t); }
	ssvh_bam_close(bam);
	vector<ssv_clip_probe> dp(probes.size());
	string text;
	for (size_t k = 0; k < probes.size(); ++k) {
		const seeksv::ClusterProbe &p = probes[k];
		ssv_clip_probe &d = dp[k];
		memset(&d, 0, sizeof(d));
		const auto it = tid_of.find(p.chr);
		d.tid = it == tid_of.end() ? -1 : it->second;
		d.lo = p.lo; d.hi = p.hi; d.side = (uint8_t)p.side; d.mode = (uint8_t)p.mode;
		if (text.size() + p.a.size() + p.b.size() >= 0xffffffffull) die("seeksv somatic -K: the tumor table's sequences are 4 GB or more");
		d.a_off = (uint32_t)text.size(); d.a_len = (uint32_t)p.a.size(); text += p.a;
		d.b_off = (uint32_t)text.size(); d.b_len = (uint32_t)p.b.size(); text += p.b;
	}
	pt.lap("tumor_table+probes");
	RunSession *const run = new RunSession; // (on the heap, never destroyed: see RunSession)
	run->ctx = acquire_ctx(o.device, nullptr);
	run->collect = true; run->probe_only = true;
	if (pt.on) ssv_prof_enable(run->ctx, 1); // (SSV_TIMING: the probe kernel's own time, below)
	check(run->ctx, ssv_clip_probe_set(run->ctx, dp.data(), (int64_t)dp.size(), text.data(), (uint64_t)text.size(), o.min_map_rate, (uint32_t)o.min_len_of_clipped_seq));
	pt.lap("gpu_init+probe_set");
	getclip_main(o.clip, run);
	run->collect = false;
	pt.lap("clip_pass (decode once, records kept in HBM, every pass's table probed)");
	vector<ssv_clip_probe_hit> hits(dp.size());
	int64_t passes = 0;
	check(run->ctx, ssv_clip_probe_get(run->ctx, hits.data(), &passes));
	check(run->ctx, ssv_clip_probe_set(run->ctx, nullptr, 0, nullptr, 0, o.min_map_rate, 0));
	for (size_t r = 0; r < rows.size(); ++r) {
		if (of_row[r].first >= 0) rows[r].normal_left_reads = hits[(size_t)of_row[r].first].support;
		if (of_row[r].second >= 0) rows[r].normal_right_reads = hits[(size_t)of_row[r].second].support;
	}
	if (pt.on) {
		ssv_prof_enable(run->ctx, 0);
		double ms = 0; int64_t launches = 0, units = 0;
		ssv_prof_get(run->ctx, "somatic_probe", &ms, &launches, &units);
		cerr << "[timing] (somatic -K: " << dp.size() << " probes, " << text.size() << " bytes of text, " << passes << " passes; somatic_probe kernel time " << ms << " ms in " << launches << " launches)" << endl;
	}
	pt.lap("probes (get)");
	return run;
}

static int somatic_main(const SomaticOptions &o)
{
	PhaseTimer pt;
	if (o.verify_crc) g_verify_crc = true;
	RunSession *run = nullptr;  // -K: the session that holds the normal's records ...
	vector<SomaticRow> probed;  // ... and the rows with their look-ups done
	if (o.from_bam) {
		run = somatic_clip_pass(o, probed, pt);
		if (!o.dump_lookups.empty()) { dump_lookups(o.dump_lookups, probed); ssv_sync(run->ctx); return 0; }
	}
	// The normal sample's clusters (all host threads: inflate + parse of a 30x sample's 5.5 M rows) are read BESIDE the GPU's work: what a row of the
	// tumor's table asks of the BAM (somatic.cpp:111,142: whether FindDiscordantReadPairs runs for it) depends on the insert size only, not on the look-ups.
	NormalClusters normal;
	string load_warnings, load_err;
	auto load = [&] { load_err = load_normal_clusters(o.clipped_file, o.min_len_of_clipped_seq, normal, load_warnings); };
	if (!run && !o.dump_lookups.empty()) {
		load();
		if (!load_err.empty()) die(load_err);
		cerr << load_warnings;
		pt.lap("normal_clusters");
		vector<SomaticRow> rows;
		string err = scan_tumor_table(o.tumor_file, normal.clip3, normal.clip5, o.offset, o.min_map_rate, 1, rows);
		if (!err.empty()) die(err);
		dump_lookups(o.dump_lookups, rows);
		return 0;
	}
	std::thread loader;
	if (!run) loader = std::thread(load);
	struct Joiner { std::thread &t; ~Joiner() { if (t.joinable()) t.join(); } } joiner{loader}; // (die() leaves through _exit; a return must not leave the thread behind)
	ssv_ctx *ctx = nullptr;
	auto get_ctx = [&] { if (!ctx) ctx = acquire_ctx(o.device, run); return ctx; }; // (main() started it; -K: the session's)
	int mean_insert_size = 0, deviation = 0;
	IsizeCarry carry;
	string isize_report; // ReadsClipReads' warnings come first on the reference's stderr (seeksv.cpp:392-398): the lines wait for the loader
	// -N n: the tally over the normal BAM is split like `getsv -N`'s (SSV_GROUP_RCCL_ONE=1: `-N 1` takes that path too, through a one-rank RCCL communicator);
	// the insert-size pass stays on rank 0, and leaves no open source behind - the ranks read their own ranges
	// -K: both passes run over the session's batches where they lie, as getsv's do inside `seeksv run`
	const bool ranks_path = !run && (o.n_ranks > 1 || getenv("SSV_GROUP_RCCL_ONE"));
	const bool device_inflate = run ? true : o.device_inflate;
	if (o.read_pair_used >= 100000) insert_size_pass(get_ctx, o.normal_bam_file, device_inflate, o.min_mapQ, o.read_pair_used, mean_insert_size, deviation, ranks_path ? nullptr : &carry, run, &isize_report);
	get_ctx();
	pt.lap("isize_pass (+ what was left of the context's start-up)");

	ofstream fout(o.somatic_file.c_str());
	if (!fout) die("Error: Cannot open output file " + o.somatic_file);
	ssvh_bam *bam = nullptr;
	if (ssvh_bam_open(o.normal_bam_file.c_str(), &bam) != 0) die("[main_samview] fail to open file for reading.");
	vector<SomaticRow> rows;
	{
		string err = parse_tumor_table(o.tumor_file, mean_insert_size, rows);
		if (!err.empty()) { if (loader.joinable()) loader.join(); if (!load_err.empty()) die(load_err); cerr << load_warnings << isize_report; die(err); }
		if (run) { // the same file parsed again, now with the insert size: the look-ups are the clip pass's
			if (rows.size() != probed.size()) die("seeksv somatic -K: the tumor table changed while it was read");
			for (size_t r = 0; r < rows.size(); ++r) { rows[r].normal_left_reads = probed[r].normal_left_reads; rows[r].normal_right_reads = probed[r].normal_right_reads; }
		}
	}
	pt.lap("tumor_table");

	// every row that asks for FindDiscordantReadPairs (getsv.cpp:1123-1247) becomes one junction of a single pass over the normal BAM
	vector<ssvh_junction_in> J;
	vector<size_t> row_of;
	for (size_t r = 0; r < rows.size(); ++r) {
		if (rows[r].kind != SomaticRow::JUNCTION || !rows[r].tally) continue;
		J.push_back(ssvh_junction_in{rows[r].up_chr.c_str(), rows[r].down_chr.c_str(), rows[r].up_pos, rows[r].down_pos, rows[r].up_strand, rows[r].down_strand});
		row_of.push_back(r);
	}
	vector<int32_t> abnormal(J.size() + 1, 0);
	if (!J.empty()) {
		const int times = 4; // seeksv.cpp:406
		ssvh_plan *plan = nullptr;
		ssvh_plan_create(bam, J.data(), (int64_t)J.size(), nullptr, nullptr, 0, mean_insert_size, deviation, times, 200, &plan);
		int64_t nj;
		const ssv_junction *dj = ssvh_plan_junctions(plan, &nj);
		vector<int32_t> counts((size_t)nj + 1, 0);
		RanksTally T; // counts only: no windows, hence nothing to replay
		T.bam_path = o.normal_bam_file; T.device_inflate = device_inflate;
		memset(&T.gp, 0, sizeof(T.gp));
		T.gp.junctions = dj; T.gp.n_junctions = nj;
		T.gp.mean = mean_insert_size; T.gp.sd = deviation; T.gp.times = times; T.gp.disc_min_mapq = o.min_mapQ;
		T.gp.n_windows = 0; T.gp.depth_min_mapq = o.min_mapQ;
		T.gp.n_targets = ssvh_bam_n_targets(bam); T.gp.target_len = ssvh_bam_target_lens(bam);
		T.n_counts = (size_t)nj; T.counts = counts.data();
		tally_records(ctx, T, ranks_path ? o.n_ranks : 0, o.devices, carry, run);
		vector<int32_t> prev(J.size() + 1, 0); // a row whose left contig is not in the normal's header reports 0
		ssvh_plan_fold(plan, counts.data(), prev.data(), nullptr, nullptr, abnormal.data(), nullptr, nullptr, nullptr, nullptr, nullptr);
		ssvh_plan_destroy(plan);
	} else carry.drop(ctx);
	pt.lap("discordant_pass");
	if (loader.joinable()) loader.join();
	if (!load_err.empty()) die(load_err);
	cerr << load_warnings << isize_report;
	pt.lap("normal_clusters (wait: read beside the passes)");
	if (!run) probe_normal_clusters(rows, normal.clip3, normal.clip5, o.offset, o.min_map_rate);
	pt.lap("cluster_lookups");
	pt.lap("discordant_pass");
	size_t k = 0;
	for (size_t r = 0; r < rows.size(); ++r) {
		const SomaticRow &row = rows[r];
		if (row.kind == SomaticRow::HEADER) { fout << row.text << endl; continue; }
		if (row.kind == SomaticRow::MESSAGE) { cerr << row.text << endl; continue; }
		int normal_abnormal = 0;
		if (row.tally) {
			if (k < row_of.size() && row_of[k] == r) normal_abnormal = abnormal[k++];
			bool known = false;
			for (int32_t t = 0, nt = ssvh_bam_n_targets(bam); t < nt && !known; ++t) known = row.up_chr == ssvh_bam_target_name(bam, t);
			if (!known) cerr << "Cannot find " << row.up_chr << ", please check whether you input a wrong file" << endl;
		}
		fout << row.text << '\t' << row.normal_left_reads << '\t' << row.normal_right_reads << '\t' << normal_abnormal << endl;
	}
	pt.lap("output");
	if (run && kCleanExit) for (auto &b : run->batches) ssv_batch_release(ctx, &b);
	release_ctx(ctx, nullptr);
	ssvh_bam_close(bam);
	pt.lap("teardown");
	return 0;
}

static int cmd_somatic(int argc, char **argv) { return somatic_main(parse_somatic(argc, argv)); }

// ---------------------------------------------------------------------------------------------------------------------
// seeksv realign: prefix.clip.fq.gz -> prefix.clip.bam.  The reference's pipeline runs an external aligner here
// (README.md:22-34, example/seeksv.sh:3: `bwa mem ref.fa prefix.clip.fq.gz | samtools view -Sb - > prefix.clip.bam`); this is the
// stand-in for hosts without bwa (ssv_realign_*, include/seeksv_hip.h): one record per clipped sequence (with -S: followed by up to INT secondary records of its other loci), in FASTQ order, the
// read name is the sequence.  No gapped alignment unless -g asks for it (one insertion or deletion of up to 16 bases per record).  The default (hash) index is meant for references that behave like random sequence (synthetic
// genomes); -c selects the sorted index, which keeps every copy of a repeat, skips seeds with more occurrences than the cap and follows the rarest first.
// -P takes WHOLE reads (e.g. getclip's prefix.unmapped_[12].fq.gz) in the place of `bwa bwasw`: the read name is the FASTQ name, and a read that is two
// stretches of two loci gets a supplementary record (flag 2048) for its second piece behind its own - what `seeksv getsv -F` reads.
// ---------------------------------------------------------------------------------------------------------------------
[[noreturn]] static void usage_realign()
{
	cerr << "Usage: seeksv realign [options] <reference fasta(.gz)> <input clipped reads (*.clip.fq.gz)> <output clip.bam>\n\n"
	     << "         -c <int>              skip seeds with more than INT occurrences; selects the sorted index (1..65535; bwa mem's -c, there 500) [hash index, no cap]\n"
	     << "         -g                    allow one insertion or deletion of 1..16 bases per alignment (M, I / D, M; gap open 6, extend 1) [ungapped]\n"
	     << "         -S <int>              also write up to INT other loci of a sequence as secondary records (flag 256, MAPQ 0; 1..16; score >= 30 and >= 0.8 x the primary's) [none]\n"
	     << "         -P                    the input holds whole reads (e.g. prefix.unmapped_[12].fq.gz): read name = FASTQ name, and a read's second piece of another\n"
	     << "                               locus follows it as a supplementary record (flag 2048, own MAPQ, S M S, never H) - the input of getsv -F; not with -g or -S [off]\n"
	     << "         -G <int>              GPU ordinal [0]" << endl;
	exit(1);
}

// -c of `seeksv realign` (and of `seeksv run -a`): 0 = not a cap
static int parse_max_occ(const char *arg)
{
	char *end = nullptr;
	const long v = strtol(arg, &end, 10);
	return (end != arg && *end == 0 && v >= 1 && v <= 65535) ? (int)v : 0;
}

// for_run: the words of `seeksv run -a` - -P is not one of them (it is run's own), and no operands
struct RealignOptions {
	int gpu = 0, max_occ = 0, max_alt = 0; // -c: 0 = the hash index; -S: 0 = no secondary records
	bool gpu_given = false, gapped = false, split = false;
	string fasta, fq, out_bam;
};

static RealignOptions parse_realign(int argc, char **argv, bool for_run = false)
{
	RealignOptions o;
	int c;
	optind = 0;
	while ((c = getopt(argc, argv, "G:c:gS:P")) != -1) {
		if (c == 'G') { o.gpu = atoi(optarg); o.gpu_given = true; }
		else if (c == 'g') o.gapped = true;
		else if (c == 'P') { if (for_run) usage_realign(); o.split = true; }
		else if (c == 'S') {
			char *end = nullptr;
			const long v = strtol(optarg, &end, 10);
			if (end == optarg || *end != 0 || v < 1 || v > 16) usage_realign();
			o.max_alt = (int)v;
		}
		else if (c == 'c') { if (!(o.max_occ = parse_max_occ(optarg))) usage_realign(); }
		else usage_realign();
	}
	if (o.split && (o.gapped || o.max_alt > 0)) usage_realign();
	if (argc - optind != (for_run ? 0 : 3)) usage_realign();
	if (!for_run) { o.fasta = argv[optind]; o.fq = argv[optind + 1]; o.out_bam = argv[optind + 2]; }
	return o;
}

static bool gz_getline(gzFile f, string &line)
{
	line.clear();
	char buf[1 << 16];
	while (gzgets(f, buf, sizeof(buf))) {
		line += buf;
		if (!line.empty() && line.back() == '\n') { line.pop_back(); if (!line.empty() && line.back() == '\r') line.pop_back(); return true; }
	}
	return !line.empty();
}

// A plain (not gzip'ed) FASTA file through all host threads: the file is mapped, cut into pieces at line starts; every piece counts its bases,
// a running sum gives each piece its first base index, then the pieces write their 2-bit codes (the words that two pieces share are OR-ed
// in atomically).  One thread parsing character by character took 2.8 s for an eighth of a human genome.  Same result as the serial loop
// (anything but ACGT becomes the same position-dependent pseudo-random base).  false: not a plain file (the caller reads it through zlib).
// base character -> 2-bit code, 4 for anything that is not A, C, G or T (either case)
static const struct BaseCode { uint8_t v[256]; BaseCode() { memset(v, 4, sizeof(v)); v['A'] = v['a'] = 0; v['C'] = v['c'] = 1; v['G'] = v['g'] = 2; v['T'] = v['t'] = 3; } uint8_t operator[](unsigned char c) const { return v[c]; } } kBaseCode;

static bool parse_fasta_parallel(const string &path, vector<string> &names, vector<int32_t> &lens, vector<int64_t> &offs, vector<uint64_t> &words)
{
	int fd = ::open(path.c_str(), O_RDONLY);
	if (fd < 0) return false;
	struct stat st;
	if (fstat(fd, &st) != 0 || st.st_size < 2) { ::close(fd); return false; }
	const size_t size = (size_t)st.st_size;
	const char *t = static_cast<const char *>(mmap(nullptr, size, PROT_READ, MAP_PRIVATE, fd, 0));
	::close(fd);
	if (t == MAP_FAILED) return false;
	if ((unsigned char)t[0] == 0x1f && (unsigned char)t[1] == 0x8b) { munmap(const_cast<char *>(t), size); return false; } // gzip
	const int nt = std::max(1, std::min(ssv::effective_cpus(), 64));
	const size_t n_pieces = std::max<size_t>(1, std::min<size_t>((size_t)nt * 8, size / (1 << 20) + 1));
	vector<size_t> cut(n_pieces + 1, size);
	cut[0] = 0;
	for (size_t k = 1; k < n_pieces; ++k) { // the line start at or behind the k-th share of the file
		size_t p = size * k / n_pieces;
		const void *nl = p < size ? memchr(t + p, '\n', size - p) : nullptr;
		cut[k] = nl ? (size_t)(static_cast<const char *>(nl) - t) + 1 : size;
	}
	struct Hdr { size_t at; int64_t bases_before_in_piece; string name; };
	vector<int64_t> n_bases(n_pieces, 0);
	vector<vector<Hdr>> hdrs(n_pieces);
	auto run = [&](auto fn) {
		std::atomic<size_t> next{0};
		vector<std::thread> th;
		auto work = [&] { for (size_t k; (k = next.fetch_add(1)) < n_pieces;) fn(k); };
		for (int w = 1; w < nt; ++w) th.emplace_back(work);
		work();
		for (auto &x : th) x.join();
	};
	run([&](size_t k) { // pass 1: bases and header lines of piece k
		int64_t nb = 0;
		for (size_t p = cut[k]; p < cut[k + 1];) {
			const void *nl = memchr(t + p, '\n', cut[k + 1] - p);
			const size_t e = nl ? (size_t)(static_cast<const char *>(nl) - t) : cut[k + 1];
			if (t[p] == '>') {
				size_t w = p + 1;
				while (w < e && t[w] != ' ' && t[w] != '\t' && t[w] != '\r') ++w;
				hdrs[k].push_back(Hdr{p, nb, string(t + p + 1, w - p - 1)});
			} else {
				size_t len = e - p;
				if (len && t[e - 1] == '\r') --len;
				nb += (int64_t)len;
			}
			p = e + 1;
		}
		n_bases[k] = nb;
	});
	vector<int64_t> first(n_pieces + 1, 0);
	for (size_t k = 0; k < n_pieces; ++k) first[k + 1] = first[k] + n_bases[k];
	const int64_t total = first[n_pieces];
	if (hdrs[0].empty() || hdrs[0][0].at != 0) { munmap(const_cast<char *>(t), size); if (total == 0 && hdrs[0].empty()) return false; die("Reference file " + path + " does not start with a '>' line"); }
	for (size_t k = 0; k < n_pieces; ++k)
		for (const Hdr &h : hdrs[k]) {
			if (!names.empty()) { lens.push_back((int32_t)(first[k] + h.bases_before_in_piece - offs.back())); offs.push_back(first[k] + h.bases_before_in_piece); }
			names.push_back(h.name);
		}
	lens.push_back((int32_t)(total - offs.back())); offs.push_back(total);
	words.assign((size_t)((total + 31) / 32) + 1, 0);
	run([&](size_t k) { // pass 2: the codes of piece k
		int64_t n = first[k];
		const int64_t n_end = first[k + 1];
		uint64_t cur = 0;
		auto flush = [&](int64_t word) { if (cur) { if (word == first[k] / 32 || word == (n_end - 1) / 32) __atomic_fetch_or(&words[(size_t)word], cur, __ATOMIC_RELAXED); else words[(size_t)word] = cur; cur = 0; } };
		for (size_t p = cut[k]; p < cut[k + 1];) {
			const void *nl = memchr(t + p, '\n', cut[k + 1] - p);
			const size_t e = nl ? (size_t)(static_cast<const char *>(nl) - t) : cut[k + 1];
			if (t[p] != '>') {
				size_t stop = e;
				if (stop > p && t[stop - 1] == '\r') --stop;
				// (a table look-up per base: a switch on random bases is a mispredicted branch for three bases in four - 12 cycles a base, 14 CPU-seconds
				// for a human genome, beside getclip on the same 16 CPUs in `seeksv run`)
				for (size_t i = p; i < stop; ++i, ++n) {
					uint64_t two = kBaseCode[(unsigned char)t[i]];
					if (two > 3) { const uint64_t h = (uint64_t)n * 0x9E3779B97F4A7C15ull; two = (h >> 61) & 3; }
					cur |= two << (2 * (n & 31));
					if ((n & 31) == 31) flush(n / 32);
				}
			}
			p = e + 1;
		}
		if (n > first[k] && (n & 31) != 0) flush((n - 1) / 32);
	});
	munmap(const_cast<char *>(t), size);
	return true;
}

// the reference: names, lengths, 2-bit bases (anything but ACGT becomes a position-dependent pseudo-random base, like bwa's index)
struct Reference { vector<string> names; vector<int32_t> lens; vector<int64_t> offs = vector<int64_t>(1, 0); vector<uint64_t> words; };
// (pre: `seeksv run` started reading this file beside getclip - the thread is joined and what it parsed is taken)
static void read_reference(const string &fasta, Reference &R, PrereadFasta *pre = nullptr)
{
	vector<string> &names = R.names; vector<int32_t> &lens = R.lens; vector<int64_t> &offs = R.offs; vector<uint64_t> &words = R.words;
	const bool fasta_check = getenv("SSV_FASTA_CHECK") != nullptr; // (tests: the serial reader runs too and must agree)
	vector<string> p_names; vector<int32_t> p_lens; vector<int64_t> p_offs(1, 0); vector<uint64_t> p_words;
	bool parsed;
	if (pre && pre->th.joinable()) {
		pre->th.join();
		parsed = pre->ok;
		p_names.swap(pre->names); p_lens.swap(pre->lens); p_offs.swap(pre->offs); p_words.swap(pre->words);
	} else parsed = parse_fasta_parallel(fasta, p_names, p_lens, p_offs, p_words);
	if (parsed && !fasta_check) { names.swap(p_names); lens.swap(p_lens); offs.swap(p_offs); words.swap(p_words); }
	else {
		gzFile f = gzopen(fasta.c_str(), "rb");
		if (!f) die("Cannot open reference file " + fasta);
		string line;
		int64_t n = 0;
		auto push = [&](uint64_t two) { if ((n & 31) == 0) words.push_back(0); words.back() |= two << (2 * (n & 31)); ++n; };
		while (gz_getline(f, line)) {
			if (line.empty()) continue;
			if (line[0] == '>') {
				if (!names.empty()) { lens.push_back((int32_t)(n - offs.back())); offs.push_back(n); }
				size_t e = line.find_first_of(" \t");
				names.push_back(line.substr(1, e == string::npos ? string::npos : e - 1));
			} else {
				if (names.empty()) die("Reference file " + fasta + " does not start with a '>' line");
				for (char ch : line) {
					uint64_t two;
					switch (ch) {
					case 'A': case 'a': two = 0; break;
					case 'C': case 'c': two = 1; break;
					case 'G': case 'g': two = 2; break;
					case 'T': case 't': two = 3; break;
					default: { uint64_t h = (uint64_t)n * 0x9E3779B97F4A7C15ull; two = (h >> 61) & 3; }
					}
					push(two);
				}
			}
		}
		gzclose(f);
		if (names.empty()) die("No sequence in reference file " + fasta);
		lens.push_back((int32_t)(n - offs.back())); offs.push_back(n);
		words.push_back(0);
	}
	if (parsed && fasta_check && (names != p_names || lens != p_lens || offs != p_offs || words != p_words)) die("[seeksv] SSV_FASTA_CHECK: the parallel FASTA reader disagrees with the serial one");
}

// clip.bam's records as arrays (read name = sequence as given; SEQ / QUAL reverse-complemented / reversed for reverse-strand hits)
struct Line { char *p; int n; }; // a NUL-terminated line of FASTQ text, where it lies
struct AlignedRecords {
	vector<int32_t> tid, pos, lq, mtid, mpos, isz;
	vector<uint16_t> flag, ncig;
	vector<uint8_t> mapq, seqqual;
	vector<uint32_t> cig_off, cig;
	vector<uint64_t> seq_off;
	vector<const char *> qn;
	int64_t n_aligned = 0, n_masked = 0, n_over = 0, n_gapped = 0; // (n_masked, n_over: SSV_RA_F_* of the sorted index; n_gapped: records with an I / D, -g)
	int64_t n_secondary = 0, n_with_alt = 0, n_cut = 0; // -S: secondary records, sequences that have any, sequences with SSV_RA_F_ALT_CUT
	int64_t n_split = 0; // -P: supplementary records = reads with a mate piece
	int64_t size() const { return (int64_t)tid.size(); }
};
// the sequences through the aligner (ssv_realign_query, or ssv_realign_query_gapped when `gapped`) and their records appended to `out`; max_alt > 0
// (ssv_realign_query_alts): behind a sequence's record its alternates in the rule's order, as secondary records.  names != nullptr (-P: ungapped, no
// alternates; ssv_realign_query_split): the records carry these read names, and a read's mate piece follows it as a supplementary record - laid out as a
// list of at most one "alternate" per read
static void align_lines(ssv_ctx *ctx, const vector<Line> &seqs, const vector<Line> &quals, AlignedRecords &out, bool gapped, int max_alt, const vector<Line> *names = nullptr)
{
	const int64_t n = (int64_t)seqs.size();
	if (!n) return;
	if (max_alt > 0) { // the alternates' lists are sized for the worst case, n * max_alt hits here and on the device: a file's sequences go a piece at a time
		static const int64_t piece = [] { const char *e = getenv("SSV_REALIGN_ALT_PIECE"); const long long v = e ? atoll(e) : 0; return v > 0 ? (int64_t)v : (int64_t)1 << 20; }();
		if (n > piece) {
			for (int64_t b = 0; b < n; b += piece) {
				const int64_t e = std::min(n, b + piece);
				align_lines(ctx, vector<Line>(seqs.begin() + b, seqs.begin() + e), vector<Line>(quals.begin() + b, quals.begin() + e), out, gapped, max_alt);
			}
			return;
		}
	}
	string blob;
	vector<uint64_t> soff(1, 0);
	{
		size_t total = 0;
		for (const Line &q : seqs) total += (size_t)q.n;
		blob.reserve(total);
		soff.reserve(seqs.size() + 1);
		for (const Line &q : seqs) { blob.append(q.p, (size_t)q.n); soff.push_back(blob.size()); }
	}
	vector<ssv_realign_hit> hits((size_t)n);
	vector<ssv_realign_gap> gaps((size_t)n, ssv_realign_gap{0, 0}); // (all zero without -g)
	vector<int64_t> alt_off((size_t)n + 1, 0); // (all zero without -S: sequence i is row i)
	vector<ssv_realign_hit> alts(max_alt > 0 ? (size_t)n * (size_t)max_alt : names ? (size_t)n : 0);
	const int rc = names       ? ssv_realign_query_split(ctx, blob.data(), soff.data(), n, hits.data(), alts.data())
	               : max_alt > 0 ? ssv_realign_query_alts(ctx, blob.data(), soff.data(), n, max_alt, gapped ? 1 : 0, hits.data(), gaps.data(), alt_off.data(), alts.data())
	               : gapped    ? ssv_realign_query_gapped(ctx, blob.data(), soff.data(), n, hits.data(), gaps.data())
	                           : ssv_realign_query(ctx, blob.data(), soff.data(), n, hits.data());
	if (rc != SSV_OK) die(string("[seeksv] realign query: ") + ssv_last_error(ctx));
	if (names) { // mates[n] -> the mate pieces that exist, back to back
		int64_t k = 0;
		for (int64_t i = 0; i < n; ++i) {
			if (alts[(size_t)i].tid >= 0) alts[(size_t)k++] = alts[(size_t)i];
			alt_off[(size_t)i + 1] = k;
		}
		out.n_split += k;
	}
	const size_t at = (size_t)out.size();
	const size_t rows = (size_t)(n + alt_off[(size_t)n]); // sequence i: rows i + alt_off[i] (its own record) .. i + 1 + alt_off[i + 1]
	for (auto *v : {&out.tid, &out.pos, &out.lq}) v->resize(at + rows);
	out.mtid.resize(at + rows, -1); out.mpos.resize(at + rows, -1); out.isz.resize(at + rows, 0);
	out.flag.resize(at + rows); out.ncig.resize(at + rows); out.mapq.resize(at + rows); out.cig_off.resize(at + rows); out.seq_off.resize(at + rows); out.qn.resize(at + rows);
	int32_t *tid = out.tid.data() + at, *pos = out.pos.data() + at, *lq = out.lq.data() + at;
	uint16_t *flag = out.flag.data() + at, *ncig = out.ncig.data() + at;
	uint8_t *mapq = out.mapq.data() + at;
	uint32_t *cig_off = out.cig_off.data() + at;
	uint64_t *seq_off = out.seq_off.data() + at;
	const char **qn = out.qn.data() + at;
	auto code4 = [](char ch) -> uint8_t {
		switch (ch) { case 'A': case 'a': return 1; case 'C': case 'c': return 2; case 'G': case 'g': return 4; case 'T': case 't': return 8; default: return 15; }
	};
	auto comp4 = [](uint8_t b) -> uint8_t { return (uint8_t)(((b & 1) << 3) | ((b & 2) << 1) | ((b & 4) >> 1) | ((b & 8) >> 3)); };
	// sizes first (CIGAR operations and packed bytes per record, running sums), then every host thread fills its share of the records
	{
		uint64_t so = out.seqqual.size();
		uint32_t co = (uint32_t)out.cig.size();
		for (int64_t i = 0; i < n; ++i) {
			const ssv_realign_hit &h = hits[(size_t)i];
			const int L = seqs[(size_t)i].n;
			const bool al = h.tid >= 0;
			out.n_aligned += al ? 1 : 0;
			out.n_masked += (h.pad[0] & SSV_RA_F_MASKED) ? 1 : 0; out.n_over += (h.pad[0] & SSV_RA_F_OVERFLOW) ? 1 : 0;
			const int64_t row = i + alt_off[(size_t)i], n_alt = alt_off[(size_t)i + 1] - alt_off[(size_t)i];
			cig_off[row] = co; seq_off[row] = so;
			const bool gap = al && gaps[(size_t)i].len != 0;
			out.n_gapped += gap ? 1 : 0;
			ncig[row] = (uint16_t)(al ? 1 + (gap ? 2 : 0) + (h.q_beg > 0 ? 1 : 0) + (h.q_end < L ? 1 : 0) : 0);
			co += ncig[row]; so += ((uint64_t)L + 1) / 2 + (uint64_t)L;
			if (!names) { out.n_secondary += n_alt; out.n_with_alt += n_alt ? 1 : 0; } out.n_cut += (h.pad[0] & SSV_RA_F_ALT_CUT) ? 1 : 0;
			for (int64_t r = 1; r <= n_alt; ++r) { // the alternates: S M S
				const ssv_realign_hit &x = alts[(size_t)(alt_off[(size_t)i] + r - 1)];
				cig_off[row + r] = co; seq_off[row + r] = so;
				ncig[row + r] = (uint16_t)(1 + (x.q_beg > 0 ? 1 : 0) + (x.q_end < L ? 1 : 0));
				co += ncig[row + r]; so += ((uint64_t)L + 1) / 2 + (uint64_t)L;
			}
		}
		out.cig.resize(co, 0);
		out.seqqual.resize(so, 0);
	}
	uint32_t *const cig = out.cig.data();
	uint8_t *const seqqual = out.seqqual.data();
	{
		const int nt = (int)std::max<int64_t>(1, std::min<int64_t>({(int64_t)ssv::effective_cpus(), 64, n / 4096}));
		auto fill = [&](int w) {
			for (int64_t qi = n * w / nt, e = n * (w + 1) / nt; qi < e; ++qi)
			for (int64_t i = qi + alt_off[(size_t)qi], r = 0, last = qi + alt_off[(size_t)qi + 1]; i <= last; ++i, ++r) { // row i: the sequence's own record (r == 0), then its alternates
				const ssv_realign_hit &h = r ? alts[(size_t)(alt_off[(size_t)qi] + r - 1)] : hits[(size_t)qi];
				const char *s = seqs[(size_t)qi].p, *q = quals[(size_t)qi].p;
				const int L = seqs[(size_t)qi].n;
				const bool al = h.tid >= 0, rev = al && h.reverse, has_q = quals[(size_t)qi].n == L;
				qn[i] = names ? (*names)[(size_t)qi].p : s;
				tid[i] = al ? h.tid : -1; pos[i] = al ? h.pos : -1; lq[i] = L;
				flag[i] = (uint16_t)((al ? (rev ? 16 : 0) : 4) | (r ? (names ? 2048 : 256) : 0)); mapq[i] = al ? h.mapq : 0;
				if (al) {
					uint32_t *c = cig + cig_off[i];
					if (h.q_beg > 0) *c++ = ((uint32_t)h.q_beg << 4) | 4u;
					const ssv_realign_gap &g = r ? ssv_realign_gap{0, 0} : gaps[(size_t)qi];
					if (g.len == 0) *c++ = ((uint32_t)(h.q_end - h.q_beg) << 4) | 0u;
					else { // M, D / I, M: the hit's coordinates are those of its own orientation, which is the record's
						const int32_t j = g.len > 0 ? g.q_at : g.q_at - g.len;
						*c++ = ((uint32_t)(g.q_at - h.q_beg) << 4) | 0u;
						*c++ = g.len > 0 ? (((uint32_t)g.len << 4) | 2u) : (((uint32_t)-g.len << 4) | 1u);
						*c++ = ((uint32_t)(h.q_end - j) << 4) | 0u;
					}
					if (h.q_end < L) *c++ = ((uint32_t)(L - h.q_end) << 4) | 4u;
				}
				uint8_t *sp = seqqual + seq_off[i], *qp = sp + ((size_t)L + 1) / 2;
				for (int k = 0; k < L; ++k) {
					const uint8_t b = rev ? comp4(code4(s[L - 1 - k])) : code4(s[k]);
					sp[k >> 1] |= (k & 1) ? b : (uint8_t)(b << 4);
					const char qc = has_q ? (rev ? q[L - 1 - k] : q[k]) : '!';
					qp[k] = (uint8_t)(qc - 33);
				}
			}
		};
		vector<std::thread> th;
		for (int w = 1; w < nt; ++w) th.emplace_back(fill, w);
		fill(0);
		for (auto &x : th) x.join();
	}
}

static void write_clip_bam(const string &out_bam, const Reference &R, AlignedRecords &A)
{
	const int64_t n = A.size();
	ssv_batch_t b;
	memset(&b, 0, sizeof(b));
	b.n = n; b.mem = SSV_MEM_HOST;
	b.tid = A.tid.data(); b.pos = A.pos.data(); b.flag = A.flag.data(); b.mapq = A.mapq.data(); b.n_cigar = A.ncig.data(); b.l_qseq = A.lq.data();
	b.mtid = A.mtid.data(); b.mpos = A.mpos.data(); b.isize = A.isz.data(); b.cigar_off = A.cig_off.data(); b.cigar = A.cig.data(); b.n_cigar_total = (int64_t)A.cig.size();
	b.seq_off = A.seq_off.data(); b.seqqual = A.seqqual.data(); b.seqqual_bytes = (int64_t)A.seqqual.size() - 16;
	vector<const char *> tn;
	for (const string &x : R.names) tn.push_back(x.c_str());
	if (ssvh_bam_write_batch_named(out_bam.c_str(), tn.data(), R.lens.data(), (int32_t)R.names.size(), &b, A.qn.data(), 0, 1) != 0) die(string("[seeksv] ") + ssvh_last_error());
}

// the index `seeksv realign` / `seeksv run` asked for: max_occ == 0 the hash index, else the sorted one with that cap
static void build_realign_index(ssv_ctx *ctx, const Reference &R, int max_occ, int64_t *dropped)
{
	const int rc = max_occ ? ssv_realign_index_sorted(ctx, R.words.data(), SSV_MEM_HOST, R.offs.back(), R.offs.data(), (int32_t)R.names.size(), max_occ, nullptr)
	                       : ssv_realign_index(ctx, R.words.data(), SSV_MEM_HOST, R.offs.back(), R.offs.data(), (int32_t)R.names.size(), dropped);
	if (rc != SSV_OK) die(string("[seeksv] realign index: ") + ssv_last_error(ctx));
}

// (n_queries >= 0: the number of sequences, where the records were never laid out on the host - `seeksv run -P`)
static string realign_summary(const AlignedRecords &A, int64_t dropped, int max_occ, bool gapped, int max_alt, bool split = false, int64_t n_queries = -1)
{
	string t = "[seeksv realign] " + to_string(n_queries >= 0 ? n_queries : A.size() - A.n_secondary - A.n_split) + " clipped sequences, " + to_string(A.n_aligned) + " aligned";
	if (gapped) t += ", " + to_string(A.n_gapped) + " with a gap";
	if (!max_occ) t += dropped ? ", " + to_string(dropped) + " repetitive index positions dropped" : string();
	else t += (A.n_masked ? ", " + to_string(A.n_masked) + " with repetitive seeds masked" : string()) + (A.n_over ? ", " + to_string(A.n_over) + " over the candidate limit" : string());
	if (max_alt) t += ", " + to_string(A.n_secondary) + " secondary records for " + to_string(A.n_with_alt) + " sequences (" + to_string(A.n_cut) + " cut at -S)";
	if (split) t += ", " + to_string(A.n_split) + " split reads (mate pieces written)";
	return t;
}

static void resident_alignments(const RunSession &run, seeksv::AlnRecords &R)
{
	const AlignedRecords &A = *run.aln.rec;
	R.n = A.size(); R.tid = A.tid.data(); R.pos = A.pos.data(); R.flag = A.flag.data(); R.n_cigar = A.ncig.data(); R.mapq = A.mapq.data();
	R.cigar_off = A.cig_off.data(); R.cigar = A.cig.data(); R.qname = A.qn.data(); R.target_names = run.aln.names;
}

static void read_fastq_lines(const string &fq, string &text, vector<Line> &seqs, vector<Line> &quals, vector<Line> *names_out);

static int realign_main(const RealignOptions &o)
{
	PhaseTimer pt;
	Reference R;
	read_reference(o.fasta, R);
	pt.lap("read reference");
	// ---- clipped sequences: the FASTQ file (its gzip members inflated side by side), cut into lines in place (the newline behind a line becomes its
	//      terminator: the sequences are the read names of the BAM records below) ----
	vector<Line> seqs, quals, names; // (names: -P only)
	string text;
	read_fastq_lines(o.fq, text, seqs, quals, o.split ? &names : nullptr);
	pt.lap("read fastq");
	ssv_ctx *ctx = acquire_ctx(o.gpu, nullptr);
	int64_t dropped = 0;
	build_realign_index(ctx, R, o.max_occ, &dropped);
	pt.lap("index");
	AlignedRecords A;
	align_lines(ctx, seqs, quals, A, o.gapped, o.max_alt, o.split ? &names : nullptr);
	pt.lap("align");
	A.seqqual.resize(A.seqqual.size() + 16, 0);
	// clip.bam is read back once, by getsv's join: its BGZF blocks are literal-only Huffman blocks (huff_gz.h: 4 x the speed of zlib level 1 on these
	// records, 1.6 x the bytes) unless SSV_BGZF_LEVEL asks for zlib
	setenv("SSV_BGZF_LEVEL", "-1", 0);
	write_clip_bam(o.out_bam, R, A);
	pt.lap("write bam");
	cerr << realign_summary(A, dropped, o.max_occ, o.gapped, o.max_alt, o.split) << endl;
	ssv_realign_free(ctx);
	release_ctx(ctx, nullptr);
	return 0;
}

static int cmd_realign(int argc, char **argv) { return realign_main(parse_realign(argc, argv)); }

// A FASTQ file (its gzip members inflated side by side) as one text, cut into lines in place (the newline behind a line becomes its terminator); names != nullptr (-P):
// the reads' names too.  `seeksv realign` and the aligner step of `seeksv run -N` read prefix.clip.fq.gz through this.
static void read_fastq_lines(const string &fq, string &text, vector<Line> &seqs, vector<Line> &quals, vector<Line> *names_out)
{
	const bool split = names_out != nullptr;
	{ const string err = seeksv::slurp_gz(fq, text); if (!err.empty()) die("Cannot open clipped reads file " + fq); }
	{
		char *base = text.empty() ? nullptr : &text[0];
		const size_t size = text.size();
		size_t at = 0;
		auto line = [&](Line &out) { // like gz_getline: a line ends at '\n' (a '\r' in front of it is dropped); a last line without one counts when it is not empty
			if (at >= size) return false;
			char *b = base + at;
			char *e = static_cast<char *>(memchr(b, '\n', size - at));
			size_t len = e ? (size_t)(e - b) : size - at;
			at += len + (e ? 1 : 0);
			if (e) { *e = 0; if (len && b[len - 1] == '\r') b[--len] = 0; }
			out.p = b; out.n = (int)len;
			return e != nullptr || len != 0;
		};
		Line l1, l2, l3, l4;
		while (line(l1)) {
			if (!line(l2) || !line(l3) || !line(l4)) die("Truncated FASTQ record in " + fq);
			if (l1.n == 0 || l1.p[0] != '@' || l3.n == 0 || l3.p[0] != '+') die("Malformed FASTQ record in " + fq);
			seqs.push_back(l2); quals.push_back(l4);
			if (split) { // the read's name: behind '@' up to the first white space ("/1" and "/2" stay)
				int k = 1;
				while (k < l1.n && l1.p[k] != ' ' && l1.p[k] != '\t') ++k;
				l1.p[k] = 0;
				names_out->push_back(Line{l1.p + 1, k - 1});
			}
		}
	}
}

// `seeksv run`: the aligner step beside getclip.  A thread with a context of its own (a second stream on the same GPU) builds the index as soon as the
// reference is read - getclip is still inflating the BAM then - and takes every pass's clipped sequences as getclip's output thread writes them out:
// when the last record of the BAM has been scanned, all but the last pass's sequences are aligned (0.7 s of a 3.7 s whole-genome run came after getclip
// before).  The records equal `seeksv realign`'s on the finished prefix.clip.fq.gz: same sequences, same order, one query per sequence.
struct RunAligner {
	std::thread th;
	std::mutex mu;
	std::condition_variable cv;
	struct Work { vector<RunSession::Piece *> pass; vector<Line> seqs, quals; }; // a pass of getclip's pieces, or (`run -N`) lines cut out of the finished FASTQ file
	std::deque<Work> todo;
	bool done = false;
	Reference R;
	AlignedRecords A;
	int64_t dropped = 0;
	int max_occ = 0; // -a "-c INT": the sorted index
	bool gapped = false; // -a "-g"
	int max_alt = 0; // -a "-S INT": secondary records
	bool keep_index = false; // `seeksv run -P`: context and index outlive the thread, for the split leg (release_index)
	ssv_ctx *kept_ctx = nullptr;
	double t_index = 0, t_align = 0, t_wait_ref = 0;
	void start(int device, const string &fasta, PrereadFasta *pre)
	{
		th = std::thread([this, device, fasta, pre] {
			auto now = [] { return std::chrono::steady_clock::now(); };
			auto t0 = now();
			ssv_ctx *ctx = nullptr;
			if (ssv_ctx_create(device, &ctx) != SSV_OK) die(string("[seeksv] ") + ssv_last_error(nullptr));
			read_reference(fasta, R, pre);
			t_wait_ref = std::chrono::duration<double>(now() - t0).count();
			t0 = now();
			build_realign_index(ctx, R, max_occ, &dropped);
			t_index = std::chrono::duration<double>(now() - t0).count();
			for (;;) {
				Work work;
				{
					std::unique_lock<std::mutex> lk(mu);
					cv.wait(lk, [this] { return !todo.empty() || done; });
					if (todo.empty()) break;
					work = std::move(todo.front());
					todo.pop_front();
				}
				t0 = now();
				vector<Line> &seqs = work.seqs, &quals = work.quals;
				for (RunSession::Piece *p : work.pass) {
					char *base = p->fq.empty() ? nullptr : &p->fq[0];
					for (const RunSession::FqRef &r : p->reads) {
						base[r.seq_off + r.seq_len] = 0; base[r.qual_off + r.qual_len] = 0; // (the newline behind a line becomes its terminator: the file is written)
						seqs.push_back(Line{base + r.seq_off, (int)r.seq_len}); quals.push_back(Line{base + r.qual_off, (int)r.qual_len});
					}
				}
				align_lines(ctx, seqs, quals, A, gapped, max_alt);
				t_align += std::chrono::duration<double>(now() - t0).count();
			}
			A.seqqual.resize(A.seqqual.size() + 16, 0);
			if (keep_index) { ssv_sync(ctx); kept_ctx = ctx; return; }
			ssv_realign_free(ctx);
			if (kCleanExit) ssv_ctx_destroy(ctx); else ssv_sync(ctx);
		});
	}
	void release_index()
	{
		if (!kept_ctx) return;
		ssv_realign_free(kept_ctx);
		if (kCleanExit) ssv_ctx_destroy(kept_ctx); else ssv_sync(kept_ctx);
		kept_ctx = nullptr;
	}
	void submit(const vector<RunSession::Piece *> &pass)
	{
		{ std::lock_guard<std::mutex> lk(mu); todo.emplace_back(); todo.back().pass = pass; }
		cv.notify_all();
	}
	void submit_lines(vector<Line> &seqs, vector<Line> &quals) // (the text they point into stays the caller's until finish())
	{
		{ std::lock_guard<std::mutex> lk(mu); todo.emplace_back(); todo.back().seqs.swap(seqs); todo.back().quals.swap(quals); }
		cv.notify_all();
	}
	void finish()
	{
		{ std::lock_guard<std::mutex> lk(mu); done = true; }
		cv.notify_all();
		th.join();
	}
};

// `seeksv run -P`: what `cat prefix.unmapped_1.fq.gz prefix.unmapped_2.fq.gz | seeksv realign -P ref.fa - prefix.F.bam` and the -F pass of `seeksv getsv -F
// prefix.F.bam` do, without the file: the reads - file 1's, then file 2's, out of the text the side channel's sinks kept - go through the aligner's index in
// pieces of SSV_REALIGN_SPLIT_PIECE reads (1 << 22; tests make it small), ssv_realign_split_batch lays every piece's records out in HBM, and the -F pass of
// the getsv context scans them there (same GPU, same process; the call has synchronised).  A read's two records lie in one piece.  Called by cmd_getsv
// where it runs its -F pass; ssv_rt_finish and the fold into the junction map as there.
static void run_split_leg(RunAligner &aligner, RunSession *run, ssv_ctx *rt_ctx, int min_mapq, JunctionMap &junction2other)
{
	ssv_ctx *actx = aligner.kept_ctx;
	if (!actx) die("[seeksv] run -P: the aligner's index is gone");
	rt_begin_for(aligner.R.names, min_mapq, rt_ctx, false);
	static const int64_t piece = [] { const char *e = getenv("SSV_REALIGN_SPLIT_PIECE"); const long long v = e ? atoll(e) : 0; return v > 0 ? (int64_t)v : (int64_t)1 << 22; }();
	seeksv::FastqReads reads;
	vector<ssv_realign_hit> hits, mates;
	AlignedRecords S; // (the counts of the closing line only)
	int64_t n_reads = 0;
	double t_cut = 0, t_align = 0, t_scan = 0;
	auto now = [] { return std::chrono::steady_clock::now(); };
	auto secs = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double>(b - a).count(); };
	auto flush = [&] {
		const int64_t n = reads.n();
		if (!n) return;
		const auto t0 = now();
		hits.resize((size_t)n); mates.resize((size_t)n);
		ssv_batch_t b;
		ssv_names_t nm;
		if (ssv_realign_split_batch(actx, reads.seqs.data(), reads.seq_off.data(), n, reads.quals.data(), reads.names.data(), reads.name_off.data(), hits.data(), mates.data(), &b, &nm) != SSV_OK)
			die(string("[seeksv] realign query: ") + ssv_last_error(actx));
		const auto t1 = now();
		check(rt_ctx, ssv_rt_scan(rt_ctx, &b, &nm));
		check(rt_ctx, ssv_sync(rt_ctx)); // (the next piece overwrites the batch)
		t_align += secs(t0, t1); t_scan += secs(t1, now());
		for (int64_t i = 0; i < n; ++i) {
			const ssv_realign_hit &h = hits[(size_t)i];
			S.n_aligned += h.tid >= 0 ? 1 : 0; S.n_split += mates[(size_t)i].tid >= 0 ? 1 : 0;
			S.n_masked += (h.pad[0] & SSV_RA_F_MASKED) ? 1 : 0; S.n_over += (h.pad[0] & SSV_RA_F_OVERFLOW) ? 1 : 0;
		}
		n_reads += n;
		reads.clear();
	};
	// the texts are cut side by side, a group of them at a time (every one holds whole records), and put together into pieces in their order
	vector<string *> texts;
	for (auto &file : run->unmapped) for (string &text : file) texts.push_back(&text);
	const size_t group = (size_t)std::max(1, std::min(ssv::effective_cpus(), 32));
	for (size_t g = 0; g < texts.size(); g += group) {
		const auto t0 = now();
		const size_t m = std::min(group, texts.size() - g);
		vector<seeksv::FastqReads> part(m);
		vector<string> errs(m);
		auto cut = [&](size_t k) { // (room first - the strings do not grow while they are filled -, on huge pages where they are large enough for that)
			const string &text = *texts[g + k];
			seeksv::FastqReads &r = part[k];
			r.seqs.reserve(text.size() / 2); r.quals.reserve(text.size() / 2); r.names.reserve(text.size() / 8);
			ssv::thp_advise(r.seqs.data(), r.seqs.capacity()); ssv::thp_advise(r.quals.data(), r.quals.capacity()); ssv::thp_advise(r.names.data(), r.names.capacity());
			if (seeksv::fastq_all(text.data(), text.size(), r, errs[k]) >= 0) errs[k].clear();
			string().swap(*texts[g + k]);
		};
		{
			vector<std::thread> th;
			for (size_t k = 1; k < m; ++k) th.emplace_back(cut, k);
			cut(0);
			for (auto &x : th) x.join();
		}
		{ // room in the piece for what the group holds (the piece's buffers are kept from piece to piece)
			size_t sb = 0, nb = 0;
			int64_t nr = 0;
			for (const auto &r : part) { sb += r.seqs.size(); nb += r.names.size(); nr += r.n(); }
			if (reads.seqs.capacity() < reads.seqs.size() + sb) {
				reads.seqs.reserve(reads.seqs.size() + sb); reads.quals.reserve(reads.quals.size() + sb); reads.names.reserve(reads.names.size() + nb);
				reads.seq_off.reserve(reads.seq_off.size() + (size_t)nr); reads.name_off.reserve(reads.name_off.size() + (size_t)nr);
				ssv::thp_advise(reads.seqs.data(), reads.seqs.capacity()); ssv::thp_advise(reads.quals.data(), reads.quals.capacity()); ssv::thp_advise(reads.names.data(), reads.names.capacity());
			}
		}
		for (size_t k = 0; k < m; ++k) if (!errs[k].empty()) die("[seeksv] run -P: " + errs[k] + " among the unmapped pairs");
		t_cut += secs(t0, now());
		for (size_t k = 0; k < m; ++k) {
			for (int64_t i0 = 0, n = part[k].n(); i0 < n;) {
				const auto t1 = now();
				const int64_t take = std::min(n - i0, piece - reads.n());
				seeksv::fastq_append_range(reads, part[k], i0, i0 + take);
				i0 += take;
				t_cut += secs(t1, now());
				if (reads.n() == piece) flush();
			}
			part[k] = seeksv::FastqReads();
		}
	}
	for (auto &file : run->unmapped) file.clear();
	flush();
	ssv_rt_result res;
	check(rt_ctx, ssv_rt_finish(rt_ctx, &res));
	seeksv::apply_readthrough(res, aligner.R.names, junction2other);
	cerr << realign_summary(S, aligner.dropped, aligner.max_occ, false, 0, true, n_reads) << endl;
	if (getenv("SSV_TIMING")) cerr << "[timing] (run -P: " << n_reads << " reads, " << res.n_candidates << " candidates, " << res.n_pairs << " pairs; cutting the text " << t_cut << " s, split query + device rows "
	                               << t_align << " s, -F scan " << t_scan << " s)" << endl;
	aligner.release_index();
}

// ---------------------------------------------------------------------------------------------------------------------
// run: getclip -> realign -> getsv in one process (seeksv.cpp:128-329 + the pipeline's external aligner step, README.md:22-34)
// ---------------------------------------------------------------------------------------------------------------------

[[noreturn]] static void usage_run()
{
	cerr << "Usage: seeksv run [options] <input.sorted.bam> <reference fasta(.gz)> <output prefix>\n\n"
	     << "The three steps of the pipeline in one process on one GPU: `getclip` (prefix.clip.gz, prefix.clip.fq.gz, prefix.unmapped_[12].fq.gz),\n"
	     << "`realign` in the place of `bwa mem` (prefix.clip.bam), `getsv` (prefix.sv.txt, prefix.unmapped.clip.fq; filtered junctions on stdout).\n"
	     << "Every file is what the three commands write one after the other; the BAM is read, inflated and decoded ONCE, on the GPU, and its\n"
	     << "records stay in HBM for the getsv passes (80 bytes a record).  An input whose name does not end in .bam is SAM text (plain or gzip; - is\n"
	     << "standard input, e.g. `samtools view -h in.cram | seeksv run - ref.fa out`): read once, decoded on the GPU, kept the same way; not with -N.\n"
	     << "(`getsv` and `somatic` as commands of their own do not take the original alignments as SAM text.)\n\n"
	     << "Options: -c <string>           options handed to getclip, e.g. -c \"-q 5 -s\"\n"
	     << "         -v <string>           options handed to getsv, e.g. -v \"-b 5 -L 100\"\n"
	     << "         -a <string>           options handed to realign, e.g. -a \"-c 500 -g -S 8\" (the GPU is chosen by -G here)\n"
	     << "         -P                    also split-align the unmapped pairs (prefix.unmapped_1.fq.gz, then prefix.unmapped_2.fq.gz: whole reads, read name =\n"
	     << "                               FASTQ name) on the aligner's index (-c of -a applies; ungapped, -g / -S of -a stay with the clipped sequences) and seed\n"
	     << "                               junctions from their two-piece alignments as `getsv -F` does (-w of -v is its MAPQ floor): the table and stdout of\n"
	     << "                               `seeksv realign -P` on the two files + `seeksv getsv -F`, from one decode.  The records are built on the GPU and stay\n"
	     << "                               there: no prefix.F.bam is written (`seeksv realign -P` writes one); every other file is unchanged.  Not with -F in -v\n"
	     << "                               or -N in -c.\n"
	     << "         -M                    mark duplicate read pairs (flag 0x400) on the GPU while the decoded records are retained, before any pass reads a flag; every pass\n"
	     << "                               ignores marked records, as with a BAM marked beforehand.  The input must be a coordinate-sorted BAM; no file is written for it.\n"
	     << "                               This program's own rule, after `samtools rmdup`: pairs with both ends mapped; equal (contig, pos, mate contig, mate pos, strands)\n"
	     << "                               of the leftmost read; the highest sum of base qualities >= 15 stays, the earliest of equals; the mate follows its read.  Aligned\n"
	     << "                               positions, not unclipped 5' ends (Picard's): copies clipped differently are not found; single reads and pairs with an unmapped\n"
	     << "                               end are never marked; read groups / libraries are not told apart.  Not with -N above 1, not on SAM text\n"
	     << "         -D                    mark duplicate pairs (flag 0x400) by the unclipped 5' ends of both reads, in any record order: mates are joined by read name, a\n"
	     << "                               pair's key is (contig, unclipped 5' end, strand) of both reads, the highest sum of base qualities >= 15 over BOTH reads stays, of\n"
	     << "                               equals the pair that comes first in the input.  Finds copies that the aligner clipped differently, which -M does not.  Takes a BAM\n"
	     << "                               or SAM text, with or without -u.  This program's own rule, Picard's comparison in outline; no external marker was matched.\n"
	     << "                               Libraries are not told apart; which mate is first of pair is not part of the key; single reads and pairs with an unmapped end\n"
	     << "                               are never marked; a name on more than two primary records is left alone.  The clip scan waits for the whole decode (as with -u).\n"
	     << "                               Not with -M, -P or -N above 1\n"
	     << "         -u                    the input is in ANY order (an aligner's output through a pipe, read-name order): its records are coordinate sorted on the GPU, where\n"
	     << "                               the run keeps them, before any pass reads them - no `samtools sort`, no file.  A stable sort by (contig, position), unplaced\n"
	     << "                               records last, records at one place in input order (libbam 0.1.x's comparison; newer samtools also orders by strand: no external\n"
	     << "                               sorter was matched).  Every file and stdout are what `seeksv run` writes for the same records in that order, except\n"
	     << "                               prefix.unmapped_[12].fq.gz, which hold the same pairs in input order.  The sample is resident twice while it is sorted\n"
	     << "                               (2 x 80 bytes a record).  Not with -N above 1, -P or -M, and not inside -c or -v\n"
	     << "         -L <file>             keep only the records that overlap a region of this BED file (chrom, start, end, tab separated, 0-based half-open; plain text, or\n"
	     << "                               gzip when the name ends in .gz; further columns, empty lines and lines starting with #, track or browser are ignored; a contig\n"
	     << "                               that the input's header does not have is ignored and counted on stderr).  A record's interval is [pos, pos + max(reference\n"
	     << "                               span, 1)): a record without CIGAR and an unmapped read placed at its mate's position cover one base; no flag takes part;\n"
	     << "                               unplaced records overlap nothing.  The restriction runs on the GPU where the records are retained - behind -M / -D, whose flags\n"
	     << "                               come from the WHOLE input, in front of -u's sort and of every pass: every file and stdout are those of `seeksv run` on a file\n"
	     << "                               that holds the kept records with those flags - except prefix.unmapped_[12].fq.gz, which are not restricted.  After\n"
	     << "                               `samtools view -L` in outline; this program's own rule, no external tool was matched.  Not with -X or -N above 1, not inside -c\n"
	     << "         -X <file>             the same with the rule turned round: keep only the records that overlap NO region of the file (an exclude list: centromeres,\n"
	     << "                               decoys, blacklists); unplaced records stay.  Not with -L or -N above 1, not inside -c or -v\n"
	     << "         -A                    also seed junctions from the input's own supplementary alignments, as `getsv -F` does from a bwasw file: a read that spans a\n"
	     << "                               breakpoint comes from `bwa mem` / minimap2 as a primary record plus a supplementary record (flag 2048), each clipped on one side.\n"
	     << "                               Every decoded chunk goes through a split-read scan on the GPU while it is retained; the pairs fold into the junction map where\n"
	     << "                               -F's do (behind the -B rows, in front of the clip join; -w of -v is the MAPQ floor).  This program's own rule, FindJunction's\n"
	     << "                               geometry with another selection and key: a record takes part when exactly one end is S or H (hard clips count: lengths come\n"
	     << "                               from the CIGAR), it is mapped to a contig and neither secondary nor duplicate; records pair by (read name, first / second of\n"
	     << "                               pair), so mates never meet; the two records must give one read length, and one of them must hold all bases of the read - a\n"
	     << "                               hard-clipped record's seqs are read from its partner.  The pass reads the input's flags, not the marks -M / -D make in this\n"
	     << "                               run; it is not restricted by -L / -X; with -u it runs in input order; a read of three or more pieces gives what hold / pair /\n"
	     << "                               drop gives, no chaining.  Takes a BAM or SAM text, with -u, -M, -D, -L, -X.  Not with -P, -F in -v or -N above 1, not inside\n"
	     << "                               -c, -v or -a\n"
	     << "         -S                    with -A: a record that holds all bases of its read and names ONE other alignment in its SA tag (SA:Z:rname,pos,strand,CIGAR,\n"
	     << "                               mapQ,NM; as `bwa mem` and minimap2 write it) also stands for that alignment when its record is not in the input - a region\n"
	     << "                               slice, a file written with `samtools view -F 0x800`, a supplementary record that is a duplicate or below the MAPQ floor.  The\n"
	     << "                               entry is used only when the record found no real partner, so a complete input gives what -A gives.  The contig must be in\n"
	     << "                               the header, the CIGAR must have exactly one clipped end (S stands for the record's H) and mapQ must reach -w of -v; a value\n"
	     << "                               with two or more entries is counted and left alone (no chaining).  stderr reports sa_tags, sa_multi, sa_refused, virtuals,\n"
	     << "                               sa_redundant, pairs_from_sa and sa_dropped_length.  Only with -A; not inside -c, -v or -a\n"
	     << "         -N <int>              cut the BAM into N runs of records, one per GPU (ranks share GPUs when there are fewer): every rank decodes its run once and\n"
	     << "                               keeps it in its own GPU's memory, the getsv pass scans the runs where they lie and the ranks' tallies and depths meet in one\n"
	     << "                               RCCL all-gather; the aligner step runs on the first GPU.  Same files and stdout as without it.  Not with -P; -c and -v\n"
	     << "                               then take neither -N nor -G (-H inside -c sets the halo) [1]\n"
	     << "         -G <int>[,<int>...]   GPU ordinal [0]; with -N: the ranks' GPUs [all GPUs of the machine in order]" << endl;
	exit(1);
}

static int cmd_run(int argc, char **argv)
{
	int c, device = 0, n_ranks = 1;
	string clip_opts, sv_opts, aln_opts, device_list;
	bool split = false, ranks_given = false, mark_dups = false, unsorted = false, pair_dups = false, splitread = false, splitread_sa = false;
	string include_file, exclude_file;
	while ((c = getopt(argc, argv, "c:v:a:G:PN:MuDL:X:AS")) >= 0) {
		switch (c) {
		case 'A': splitread = true; break;
		case 'S': splitread_sa = true; break;
		case 'P': split = true; break;
		case 'M': mark_dups = true; break;
		case 'u': unsorted = true; break;
		case 'D': pair_dups = true; break;
		case 'L': include_file = optarg; break;
		case 'X': exclude_file = optarg; break;
		case 'c': clip_opts = optarg; break;
		case 'v': sv_opts = optarg; break;
		case 'a': aln_opts = optarg; break;
		case 'G': device = atoi(optarg); device_list = optarg; break; // (a list: its first GPU - the ranks' GPUs with -N)
		case 'N': n_ranks = atoi(optarg); ranks_given = true; break;
		default: usage_run();
		}
	}
	if (argc != optind + 3 || n_ranks < 1) usage_run();
	const vector<int> devices = ranks_given ? parse_devices(device_list.c_str()) : vector<int>();
	const bool ranked = n_ranks > 1;
	if (ranked) device = device_of_rank(0, devices);
	const string bam = argv[optind], fasta = argv[optind + 1], prefix = argv[optind + 2];
	// The three steps' options, each through the step's own parser: a usage error or a value out of range ends the run here with the step's usage text, before
	// the GPU context is asked for and before any file exists.  The GPU of realign is run's own -G.
	// -u is run's own: refused inside -c / -v with its reason, not with the steps' usage texts
	for (const string *words : {&clip_opts, &sv_opts, &aln_opts}) { // -A is run's own as well
		std::istringstream in(*words);
		for (string w; in >> w;)
			if (w == "-A") die("seeksv run: -A scans the records that this run decodes, once, on their way into GPU memory; -A inside -c, -v or -a is not supported");
	}
	if (splitread_sa) { // -S is run's own, and a mode of -A (inside -a, -S stays realign's own option when -S is not given to run)
		for (const string *words : {&clip_opts, &sv_opts, &aln_opts}) {
			std::istringstream in(*words);
			for (string w; in >> w;)
				if (w == "-S") die("seeksv run: -S reads the SA tags of the records that this run decodes, as a mode of run's own -A; -S inside -c, -v or -a is not supported with it");
		}
		if (!splitread) die("seeksv run: -S adds the SA tags' alignments to the split-read pass of -A; -S without -A is not supported");
	}
	for (const string *words : {&clip_opts, &sv_opts}) {
		std::istringstream in(*words);
		for (string w; in >> w;) {
			if (w == "-u") die("seeksv run: -u sorts the records that this run keeps, once, for all its steps; -u inside -c or -v is not supported");
			// -L / -X are run's own too (inside -v, -L is getsv's flank length as before)
			if (w == "-X" || (w == "-L" && words == &clip_opts))
				die("seeksv run: -L and -X restrict the records that this run keeps, once, for all its steps; " + w + " inside -c or -v is not supported");
		}
	}
	const RealignOptions aln = parse_words("realign", aln_opts, parse_realign);
	if (aln.gpu_given) die("seeksv run: the GPU is chosen by run's own -G, not inside -a");
	GetclipOptions clip = parse_words("getclip", clip_opts, parse_getclip);
	GetsvOptions sv = parse_words("getsv", sv_opts, parse_getsv);
	// refused before anything is written
	// -P: the pass has one source, and the ranks' getclip has another side channel
	if (ranked && !is_bam_name(bam)) die("seeksv run: -N cuts a BAM into runs of records; SAM text is read once, from its start to its end, by one GPU");
	if (split && ranked) die("seeksv run: -P takes the unmapped pairs of a single getclip pass; -N is not supported with it");
	if (split && !sv.connect_bam.empty()) die("seeksv run: -P is the -F pass of this run; -F inside -v names another source for it");
	if (split && clip.ranks_given) die("seeksv run: -P takes the unmapped pairs of a single getclip pass; -N inside -c is not supported with it");
	// -M: one stream of records in file order, decoded with every record's qualities by the BAM decoder
	if (mark_dups && ranked) die("seeksv run: -M marks duplicates in one stream of records in file order; -N above 1 is not supported with it");
	if (mark_dups && !is_bam_name(bam)) die("seeksv run: -M reads a BAM; SAM text is not supported with it");
	// -u: one stream of records kept on one GPU and sorted there
	if (unsorted && ranked) die("seeksv run: -u sorts the records that one GPU keeps; -N above 1 is not supported with it");
	if (unsorted && split) die("seeksv run: -u hands the unmapped pairs over in input order, which is not the order -P's pass takes them in from a sorted file; -P is not supported with it");
	if (unsorted && mark_dups) die("seeksv run: -u does not carry the read names through the sort, which -M's digests need; -M is not supported with it");
	// -D: one mark over the records that one GPU keeps, behind the whole decode
	if (pair_dups && mark_dups) die("seeksv run: -D and -M are two rules for the one duplicate flag; -M is not supported with -D");
	if (pair_dups && ranked) die("seeksv run: -D joins mates by name among the records that one GPU keeps; -N above 1 is not supported with it");
	if (pair_dups && split) die("seeksv run: -D defers every pass behind the whole decode, -P's pass among them; -P is not supported with it");
	// -L / -X: one list, applied where one GPU retains the records
	if (!include_file.empty() && !exclude_file.empty()) die("seeksv run: -L keeps the records inside its regions and -X those outside; -X is not supported with -L");
	if ((!include_file.empty() || !exclude_file.empty()) && ranked)
		die(string("seeksv run: ") + (include_file.empty() ? "-X" : "-L") + " restricts the records that one GPU keeps; -N above 1 is not supported with it");
	// -A: one session, fed by the one pump of one GPU
	if (splitread && split) die("seeksv run: -A and -P both feed the one split-alignment session of this run, which has one source; -P is not supported with -A");
	if (splitread && !sv.connect_bam.empty()) die("seeksv run: -A is the -F pass of this run; -F inside -v names another source for it");
	if (splitread && ranked) die("seeksv run: -A pairs the records of a read by name among the records that one GPU decodes; -N above 1 is not supported with it");
	// -N: the run cuts the file once for both steps and maps its ranks to GPUs itself
	if (ranked && (clip.ranks_given || clip.devices_given || sv.ranks_given || sv.devices_given))
		die("seeksv run: with -N the ranks and their GPUs are run's own -N and -G; -N or -G inside -c or -v is not supported with it");
	// ... and without it getclip is the single pass the aligner step and the junction stage take their input from (-v "-N n" is `getsv -N` over the file)
	if (clip.ranks_given || clip.devices_given) die("seeksv run: -N or -G inside -c is not supported; the ranks of a run and their GPUs are run's own -N and -G");
	// what run decides itself
	clip.device_inflate = true; clip.n_ranks = n_ranks; clip.device = device; clip.devices = ranked ? devices : vector<int>(1, device); // (ranks without -G take the machine's GPUs in order)
	clip.prefix = prefix; clip.bamfile = bam; clip.mark_dups = mark_dups; clip.sort_input = unsorted; clip.pair_dups = pair_dups;
	clip.splitread = splitread; clip.splitread_mapq = sv.min_mapQ2; clip.splitread_sa = splitread_sa;
	clip.regions_file = include_file.empty() ? exclude_file : include_file; clip.regions_exclude = include_file.empty() && !exclude_file.empty();
	sv.device = device; sv.devices = vector<int>(1, device);
	sv.clip_bam = prefix + ".clip.bam"; sv.original_bam = bam; sv.clipfile = prefix + ".clip.gz"; sv.breakpoint_file = prefix + ".sv.txt"; sv.clip_unmap_fq_file = prefix + ".unmapped.clip.fq";

	PhaseTimer pt;
	RunSession *const run = new RunSession;
	run->ctx = acquire_ctx(device, nullptr);
	if (ranked) {
		run->ranks.rank.resize((size_t)n_ranks);
		for (int r = 0; r < n_ranks; ++r) run->ranks.rank[(size_t)r].device = device_of_rank(r, devices);
		run->ranks.rank[0].ctx = run->ctx;
	}
	run->collect = !ranked;
	pt.lap("run: gpu_init");
	PrereadFasta &pre = run->preread;
	pre.th = std::thread([&pre, fasta] { pre.ok = parse_fasta_parallel(fasta, pre.names, pre.lens, pre.offs, pre.words); });
	RunAligner &aligner = *new RunAligner; // (never destroyed: die() may exit while its thread runs)
	aligner.max_occ = aln.max_occ; aligner.gapped = aln.gapped; aligner.max_alt = aln.max_alt;
	aligner.keep_index = split; run->keep_unmapped = split;
	aligner.start(device, fasta, &pre);
	run->on_pass = [&aligner](const vector<RunSession::Piece *> &pass) { aligner.submit(pass); };
	int rc = getclip_main(clip, run);
	run->collect = false;
	run->on_pass = nullptr;
	pt.lap("run: getclip (decode once, records kept in HBM)");
	if (pt.on && !run->batches.empty()) { // what stays resident: the same three counts give the same bytes, whichever decoder made the batches
		int64_t n = 0, ops = 0, sq = 0;
		for (const ssv_batch_t &b : run->batches) { n += b.n; ops += b.n_cigar_total; sq += b.seqqual_bytes; }
		cerr << "[timing] (run: " << n << " records kept in " << run->batches.size() << " batches, " << ops << " CIGAR operations, " << sq << " bytes of bases + qualities: "
		     << (n ? (double)(n * 64 + ops * 4 + sq) / (double)n : 0.0) << " bytes a record in lines, operations and bases)" << endl;
	}
	const RunRanks &ranks = run->ranks;
	const bool by_ranks = run->ranked(); // (fell back: from here on this is `seeksv run` without -N)
	if (by_ranks && pt.on)
		for (int r = 0; r < n_ranks; ++r)
			cerr << "[timing] (run -N rank " << r << "/" << n_ranks << ": device " << ranks.rank[(size_t)r].device << ", " << ranks.rank[(size_t)r].kept << " records kept, "
			     << ranks.parts[(size_t)r].halo_records << " halo records)" << endl;
	string fq_text; // `run -N`: prefix.clip.fq.gz read back - the aligned records' read names point into it
	if (by_ranks && rc == 0) { // the ranks' getclip hands no pass over while it runs: the aligner takes the finished file's sequences, as `seeksv realign` does
		vector<Line> seqs, quals;
		read_fastq_lines(prefix + ".clip.fq.gz", fq_text, seqs, quals, nullptr);
		aligner.submit_lines(seqs, quals);
	}
	aligner.finish();
	pt.lap("run: realign (what was left of it behind getclip)");
	// clip.bam's BGZF blocks are literal-only Huffman blocks (huff_gz.h) unless SSV_BGZF_LEVEL asks for zlib; it is written under a temporary name and renamed
	// when it is whole: a run that dies in getsv must not leave half a clip.bam where `seeksv getsv` would find it
	setenv("SSV_BGZF_LEVEL", "-1", 0);
	const string clip_bam = sv.clip_bam;
	auto aligner_lines = [&] {
		cerr << realign_summary(aligner.A, aligner.dropped, aligner.max_occ, aligner.gapped, aligner.max_alt) << endl;
		if (pt.on) cerr << "[timing] (aligner beside getclip: context + reference " << aligner.t_wait_ref << " s, index " << aligner.t_index << " s, align " << aligner.t_align << " s)" << endl;
	};
	if (by_ranks && rc == 0) {
		// the junction stage of getsv reads prefix.clip.gz and prefix.clip.bam back as files: clip.bam is written whole first, then the getsv step runs over the
		// ranks' records where they lie
		write_clip_bam(clip_bam + ".tmp", aligner.R, aligner.A);
		if (rename((clip_bam + ".tmp").c_str(), clip_bam.c_str()) != 0) die("Cannot write file " + clip_bam);
		pt.lap("run: clip.bam written");
		aligner_lines();
		sv.device_inflate = true; sv.n_ranks = n_ranks; sv.devices = devices;
		rc = getsv_main(sv, run);
	} else if (rc == 0) {
		// clip.bam is read back by nobody in this process (getsv's join takes the records from memory): it is written beside getsv, by a thread that is joined below
		run->aln.rec = &aligner.A; run->aln.names = aligner.R.names;
		run->bam_writer = std::thread([&aligner, clip_bam] { write_clip_bam(clip_bam + ".tmp", aligner.R, aligner.A); });
		aligner_lines();
		if (split) run->split_leg = [&aligner, run](ssv_ctx *rt_ctx, int min_mapq, JunctionMap &jm) { run_split_leg(aligner, run, rt_ctx, min_mapq, jm); };
		rc = getsv_main(sv, run);
		run->split_leg = nullptr;
	}
	aligner.release_index(); // (run -P whose getsv did not get as far as the leg)
	pt.lap("run: getsv (records in HBM)");
	if (run->bam_writer.joinable()) {
		run->bam_writer.join();
		if (rename((clip_bam + ".tmp").c_str(), clip_bam.c_str()) != 0) die("Cannot write file " + clip_bam);
		pt.lap("run: clip.bam written");
	}
	ssv_ctx *ctx = run->ctx;
	if (kCleanExit) run->ranks.release(); // (the ranks' batches, and every context but rank 0's - which is `ctx`)
	else for (size_t r = 1; r < ranks.rank.size(); ++r) if (ranks.rank[r].ctx) ssv_sync(ranks.rank[r].ctx);
	if (kCleanExit) {
		for (auto &b : run->batches) ssv_batch_release(ctx, &b);
		run->ctx = nullptr;
		ssv_ctx_destroy(ctx);
	} else ssv_sync(ctx);
	return rc;
}

static double wall_now() { return std::chrono::duration<double>(std::chrono::system_clock::now().time_since_epoch()).count(); }

// SSV_TIMING=2: where the command's CPU time went - the process's user + system seconds (threads that have ended included) and, of the threads still alive, the ones
// that used more than 50 ms, by name (/proc/self/task).  A box that gives a command 16 CPUs of host time bounds it by this sum.
static void cpu_report()
{
	struct rusage ru;
	if (getrusage(RUSAGE_SELF, &ru) != 0) return;
	const double hz = (double)sysconf(_SC_CLK_TCK);
	fprintf(stderr, "[timing] (cpu: user %.2f s, system %.2f s in all;", ru.ru_utime.tv_sec + ru.ru_utime.tv_usec * 1e-6, ru.ru_stime.tv_sec + ru.ru_stime.tv_usec * 1e-6);
	std::map<string, std::pair<double, int>> by_name;
	if (DIR *d = opendir("/proc/self/task")) {
		while (struct dirent *e = readdir(d)) {
			if (e->d_name[0] == '.') continue;
			FILE *f = fopen((string("/proc/self/task/") + e->d_name + "/stat").c_str(), "r");
			if (!f) continue;
			char line[1024];
			if (fgets(line, sizeof line, f)) {
				const char *l = strchr(line, '('), *r = strrchr(line, ')');
				unsigned long ut = 0, st = 0;
				if (l && r && r > l && sscanf(r + 2, "%*c %*d %*d %*d %*d %*d %*u %*u %*u %*u %*u %lu %lu", &ut, &st) == 2) {
					auto &x = by_name[string(l + 1, r)];
					x.first += (double)(ut + st) / hz; ++x.second;
				}
			}
			fclose(f);
		}
		closedir(d);
	}
	fprintf(stderr, " threads alive at the end:");
	for (auto &kv : by_name) if (kv.second.first >= 0.05) fprintf(stderr, " %s x%d %.2f s;", kv.first.c_str(), kv.second.second, kv.second.first);
	fprintf(stderr, ")\n");
}

int main(int argc, char **argv)
{
	const bool stamp = getenv("SSV_TIMING") != nullptr; // with the caller's own clock around the process: exec -> main, main -> exit, exit -> reaped
	if (stamp) fprintf(stderr, "[stamp] wall clock at main: %.6f\n", wall_now());
	if (argc == 1) usage_top();
	const string cmd = argv[1];
	if (cmd != "getclip" && cmd != "getsv" && cmd != "somatic" && cmd != "realign" && cmd != "run") {
		cerr << "[seeksv] unrecognized command '" << argv[1] << "'" << endl;
		return 1;
	}
	if (argc == 2) { if (cmd == "getclip") usage_getclip(); else if (cmd == "getsv") usage_getsv(); else if (cmd == "realign") usage_realign(); else if (cmd == "run") usage_run(); else usage_somatic(); }
	{ // the GPU context starts coming up now (the device: the first number behind a -G)
		int dev = 0;
		for (int k = 2; k + 1 < argc; ++k) if (!strcmp(argv[k], "-G")) { dev = atoi(argv[k + 1]); break; }
		bool gpu_free = false; // getsv -J stops before any BAM pass (a test hook that needs no GPU)
		for (int k = 2; k < argc; ++k) if (!strcmp(argv[k], "-J")) gpu_free = true;
		g_near_device = dev;
		if (!gpu_free && argc > 3) early_ctx_start(dev);
	}
	optind = 1; // like SelectStep (seeksv.cpp:444-452): the sub-command becomes argv[0]
	int rc;
	if (cmd == "somatic") rc = cmd_somatic(argc - 1, argv + 1);
	else if (cmd == "realign") rc = cmd_realign(argc - 1, argv + 1);
	else if (cmd == "run") rc = cmd_run(argc - 1, argv + 1);
	else rc = cmd == "getclip" ? cmd_getclip(argc - 1, argv + 1) : cmd_getsv(argc - 1, argv + 1);
	if (kCleanExit) return rc;
	cout.flush(); cerr.flush(); fflush(nullptr);
	if (stamp && atoi(getenv("SSV_TIMING")) >= 2) cpu_report();
	if (stamp) { fprintf(stderr, "[stamp] wall clock at exit: %.6f\n", wall_now()); fflush(stderr); }
	_exit(rc); // (see release_ctx)
}
