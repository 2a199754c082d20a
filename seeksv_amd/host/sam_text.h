// sam_text.h - reader of SAM text files for `getsv -F` and for getsv's clipped-sequence re-alignments (the reference opens every such name without ".bam" as
// text, "-" as standard input: process_bwasw.cpp:12-16, getsv.h:437-446).
// The header ('@' lines up to the first record; @SQ SN: / LN:) is parsed here on the host; the records are NOT: their text goes to the GPU as it is
// (ssv_samdec_decode), in chunks cut anywhere, which a reader thread fills ahead of the decoder.  Plain files are read with pread, gzip-compressed ones
// (detected by their magic bytes) with zlib's gzread: one stream on one thread - its rate has not been measured.  Standard input is read sequentially through gzread in
// either form (zlib passes plain text through).
#ifndef SEEKSV_SAM_TEXT_H_
#define SEEKSV_SAM_TEXT_H_

#include <stddef.h>
#include <stdint.h>

#include <condition_variable>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

namespace seeksv {

class SamTextReader {
public:
	typedef void *(*AllocFn)(size_t bytes); // staging memory (page-locked where the caller can); nullptr: malloc
	typedef void (*FreeFn)(void *p);
	struct Chunk {
		const uint8_t *data = nullptr;
		size_t bytes = 0;
		bool last = false; // the file ends with this chunk
	};

	SamTextReader() = default;
	~SamTextReader() { close(); }
	SamTextReader(const SamTextReader &) = delete;
	SamTextReader &operator=(const SamTextReader &) = delete;

	// opens the file ("-": standard input, plain or gzip) and reads its header; false: err says why
	bool open(const std::string &path, std::string &err);
	const std::vector<std::string> &target_names() const { return names_; }
	const std::vector<int32_t> &target_lens() const { return lens_; }
	uint64_t first_record_line() const { return first_record_line_; } // 1-based, in the file
	bool is_gzip() const { return gzip_; }

	// the reader thread: chunks of up to chunk_bytes into three buffers in turn
	void start(size_t chunk_bytes, AllocFn alloc = nullptr, FreeFn free_fn = nullptr);
	// the next chunk (blocks until it is read); the chunk handed out before becomes the reader's again.  false: the file is over (or err is set)
	bool next(Chunk &c, std::string &err);
	// the chunk behind the one next() handed out last, when the reader has finished it already (to announce it to the GPU ahead)
	bool ready_behind(Chunk &c);
	void close();

private:
	static constexpr int NS = 3;
	long raw_read(void *dst, size_t cap, std::string &err);
	void reader_main();

	int fd_ = -1;
	void *gz_ = nullptr; // gzFile (gzip files, and standard input in either form)
	bool gzip_ = false;
	uint64_t file_off_ = 0;
	std::string pending_; // what was read behind the header
	size_t pending_at_ = 0;
	std::vector<std::string> names_;
	std::vector<int32_t> lens_;
	uint64_t first_record_line_ = 1;

	struct Slot { uint8_t *p = nullptr; size_t bytes = 0; bool last = false; std::string err; } slot_[NS];
	size_t chunk_bytes_ = 0;
	AllocFn alloc_ = nullptr;
	FreeFn free_ = nullptr;
	std::thread reader_;
	std::mutex mu_;
	std::condition_variable cv_;
	int64_t produced_ = 0, released_ = 0, cur_ = 0;
	bool stop_ = false, started_ = false, over_ = false;
};

} // namespace seeksv
#endif
