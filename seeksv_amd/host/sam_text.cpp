// sam_text.cpp - see sam_text.h
#include "sam_text.h"

#include <fcntl.h>
#include <unistd.h>
#include <zlib.h>

#include <algorithm>
#include <cerrno>
#include <cstdlib>
#include <cstring>

namespace seeksv {

long SamTextReader::raw_read(void *dst, size_t cap, std::string &err)
{
	if (gz_) {
		const int n = gzread(static_cast<gzFile>(gz_), dst, (unsigned)std::min<size_t>(cap, (size_t)1 << 30));
		if (n < 0) { int e = 0; const char *m = gzerror(static_cast<gzFile>(gz_), &e); err = std::string("[seeksv] cannot read the SAM file: ") + (m ? m : "zlib error"); return -1; }
		return n;
	}
	for (;;) {
		const ssize_t n = pread(fd_, dst, cap, (off_t)file_off_);
		if (n < 0 && errno == EINTR) continue;
		if (n < 0) { err = std::string("[seeksv] cannot read the SAM file: ") + strerror(errno); return -1; }
		file_off_ += (uint64_t)n;
		return (long)n;
	}
}

// the value of a "\tXX:" field of a header line ("" when it is not there)
static std::string header_field(const std::string &line, const char *tag)
{
	size_t at = 0;
	while ((at = line.find('\t', at)) != std::string::npos) {
		++at;
		if (line.compare(at, 3, tag) == 0) {
			const size_t e = line.find('\t', at);
			return line.substr(at + 3, e == std::string::npos ? std::string::npos : e - at - 3);
		}
	}
	return "";
}

bool SamTextReader::open(const std::string &path, std::string &err)
{
	close();
	if (path == "-") {
		// standard input: a pipe has no pread and nothing may be consumed before the format is known - zlib looks at the first two bytes itself and hands plain
		// text through unchanged (gzread's transparent mode), so both forms go through gzread
		const int dupfd = dup(STDIN_FILENO);
		gzFile g = dupfd >= 0 ? gzdopen(dupfd, "rb") : nullptr;
		if (!g) { if (dupfd >= 0) ::close(dupfd); err = "cannot open standard input"; return false; }
		gzbuffer(g, 1u << 20);
		gz_ = g;
	} else {
		fd_ = ::open(path.c_str(), O_RDONLY);
		if (fd_ < 0) { err = "cannot open " + path; return false; }
		unsigned char magic[2] = {0, 0};
		const ssize_t got = pread(fd_, magic, 2, 0);
		if (got == 2 && magic[0] == 0x1f && magic[1] == 0x8b) {
			const int dupfd = dup(fd_);
			gzFile g = dupfd >= 0 ? gzdopen(dupfd, "rb") : nullptr;
			if (!g) { if (dupfd >= 0) ::close(dupfd); err = "cannot open " + path; return false; }
			gzbuffer(g, 1u << 20);
			gz_ = g;
		}
	}
	// the header: every line up to the first one that does not begin with '@'
	names_.clear(); lens_.clear(); pending_.clear(); pending_at_ = 0; file_off_ = 0;
	uint64_t line_no = 1;
	size_t line_start = 0;
	bool eof = false;
	std::vector<char> buf((size_t)1 << 16);
	for (;;) {
		// a whole line at line_start, or the end of the file
		size_t nl;
		while ((nl = pending_.find('\n', line_start)) == std::string::npos && !eof) {
			const long n = raw_read(buf.data(), buf.size(), err);
			if (n < 0) return false;
			if (n == 0) eof = true; else pending_.append(buf.data(), (size_t)n);
		}
		if (line_start >= pending_.size()) break;       // the file is over behind the header
		if (pending_[line_start] != '@') break;         // the first record
		const size_t line_end = nl == std::string::npos ? pending_.size() : nl;
		std::string line = pending_.substr(line_start, line_end - line_start);
		if (!line.empty() && line.back() == '\r') line.pop_back();
		if (line.compare(0, 3, "@SQ") == 0 && (line.size() == 3 || line[3] == '\t')) {
			const std::string sn = header_field(line, "SN:"), ln = header_field(line, "LN:");
			if (!sn.empty()) { names_.push_back(sn); lens_.push_back((int32_t)strtol(ln.c_str(), nullptr, 10)); }
		}
		line_start = nl == std::string::npos ? pending_.size() : nl + 1;
		++line_no;
	}
	first_record_line_ = line_no;
	pending_at_ = line_start;
	gzip_ = gz_ && !gzdirect(static_cast<gzFile>(gz_));
	return true;
}

void SamTextReader::start(size_t chunk_bytes, AllocFn alloc, FreeFn free_fn)
{
	chunk_bytes_ = chunk_bytes ? chunk_bytes : 1;
	alloc_ = alloc; free_ = free_fn;
	started_ = true;
	reader_ = std::thread([this] { reader_main(); });
}

void SamTextReader::reader_main()
{
	for (int64_t k = 0;; ++k) {
		{
			std::unique_lock<std::mutex> lk(mu_);
			cv_.wait(lk, [&] { return stop_ || k - released_ < NS; });
			if (stop_) break;
		}
		Slot &S = slot_[k % NS];
		S.bytes = 0; S.last = false; S.err.clear();
		if (!S.p) S.p = static_cast<uint8_t *>(alloc_ ? alloc_(chunk_bytes_ + 64) : malloc(chunk_bytes_ + 64));
		if (!S.p) S.err = "[seeksv] out of memory (SAM staging buffer)";
		while (S.err.empty() && S.bytes < chunk_bytes_) {
			if (pending_at_ < pending_.size()) { // what the header's reads took along
				const size_t n = std::min(chunk_bytes_ - S.bytes, pending_.size() - pending_at_);
				memcpy(S.p + S.bytes, pending_.data() + pending_at_, n);
				S.bytes += n; pending_at_ += n;
				if (pending_at_ == pending_.size()) { std::string().swap(pending_); pending_at_ = 0; }
				continue;
			}
			const long n = raw_read(S.p + S.bytes, chunk_bytes_ - S.bytes, S.err);
			if (n < 0) break;
			if (n == 0) { S.last = true; break; }
			S.bytes += (size_t)n;
		}
		const bool done = S.last || !S.err.empty();
		{
			std::lock_guard<std::mutex> lk(mu_);
			produced_ = k + 1;
		}
		cv_.notify_all();
		if (done) break;
	}
}

bool SamTextReader::next(Chunk &c, std::string &err)
{
	if (!started_ || over_) return false;
	{
		std::unique_lock<std::mutex> lk(mu_);
		if (cur_ > 0) released_ = cur_; // the chunk handed out before
		cv_.notify_all();
		cv_.wait(lk, [&] { return produced_ > cur_; });
	}
	Slot &S = slot_[cur_ % NS];
	++cur_;
	if (!S.err.empty()) { err = S.err; over_ = true; return false; }
	c.data = S.p; c.bytes = S.bytes; c.last = S.last;
	if (S.last) over_ = true;
	return true;
}

bool SamTextReader::ready_behind(Chunk &c)
{
	if (!started_ || over_) return false;
	{
		std::lock_guard<std::mutex> lk(mu_);
		if (produced_ <= cur_) return false;
	}
	Slot &S = slot_[cur_ % NS];
	if (!S.err.empty() || !S.bytes) return false;
	c.data = S.p; c.bytes = S.bytes; c.last = S.last;
	return true;
}

void SamTextReader::close()
{
	if (started_) {
		{ std::lock_guard<std::mutex> lk(mu_); stop_ = true; }
		cv_.notify_all();
		if (reader_.joinable()) reader_.join();
		started_ = false;
	}
	for (auto &S : slot_) { if (S.p) { if (free_) free_(S.p); else if (!alloc_) free(S.p); } S.p = nullptr; S.bytes = 0; }
	if (gz_) { gzclose(static_cast<gzFile>(gz_)); gz_ = nullptr; }
	if (fd_ >= 0) { ::close(fd_); fd_ = -1; }
	stop_ = false; over_ = false; produced_ = released_ = cur_ = 0;
	pending_.clear(); pending_at_ = 0;
}

} // namespace seeksv
