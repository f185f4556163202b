// imageio.cpp — float image output for HDRFilm::develop (the reference goes through OpenImageIO,
// src/librender/image.cpp:20-43): PFM and uncompressed scanline OpenEXR (32-bit float channels); image input for the
// `bitmap` texture: PFM and binary PGM / PPM.
#include <misaki/render.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <fstream>

namespace misaki {

void write_pfm(const std::string &path, int w, int h, int channels, const float *data) {
    if (channels != 1 && channels != 3) Throw("write_pfm(): 1 or 3 channels expected");
    std::ofstream os(path, std::ios::binary);
    if (!os) Throw("Could not open \"{}\" for writing", path);
    os << (channels == 3 ? "PF" : "Pf") << "\n" << w << " " << h << "\n-1.0\n";   // little endian, bottom-up rows
    for (int y = h - 1; y >= 0; --y) os.write((const char *) (data + (size_t) y * w * channels), (std::streamsize) sizeof(float) * w * channels);
}

namespace {
// one header token of a PNM / PFM file: whitespace and '#' comments skipped; empty at the end of the file
std::string header_token(std::istream &is) {
    std::string t;
    int c;
    while ((c = is.get()) != EOF) {
        if (c == '#') { while ((c = is.get()) != EOF && c != '\n') {} continue; }
        if (!std::isspace(c)) { t.push_back((char) c); break; }
    }
    while ((c = is.get()) != EOF && !std::isspace(c)) t.push_back((char) c);      // (consumes the ONE whitespace after the token)
    return t;
}
// IEC 61966-2-1: encoded value in [0, 1] -> linear, in double, rounded once
float srgb_to_linear(double v) { return (float) (v <= 0.04045 ? v / 12.92 : std::pow((v + 0.055) / 1.055, 2.4)); }
}  // namespace

void read_image(const std::string &path, bool raw, int &w, int &h, std::vector<float> &rgb) {
    std::ifstream is(path, std::ios::binary);
    if (!is) Throw("Could not open the image file \"{}\"", path);
    const std::string magic = header_token(is);
    const bool pfm = magic == "PF" || magic == "Pf", pnm = magic == "P5" || magic == "P6";
    if (!pfm && !pnm) Throw("\"{}\": not a PFM or binary PGM / PPM image (magic number \"{}\")", path, magic.substr(0, 8));
    const int channels = (magic == "PF" || magic == "P6") ? 3 : 1;
    const std::string ws = header_token(is), hs = header_token(is), third = header_token(is);
    char *end = nullptr;
    const long lw = std::strtol(ws.c_str(), &end, 10), lh = std::strtol(hs.c_str(), nullptr, 10);
    const double scale = std::strtod(third.c_str(), &end);
    if (third.empty() || lw < 1 || lh < 1 || lw > 65536 || lh > 65536 || end == third.c_str())
        Throw("\"{}\": truncated or invalid image header", path);
    w = (int) lw; h = (int) lh;
    const size_t n = (size_t) w * h * channels;
    rgb.assign((size_t) w * h * 3, 0.f);
    auto put = [&](size_t pixel, int c, float v) { if (channels == 3) rgb[pixel * 3 + c] = v; else rgb[pixel * 3] = rgb[pixel * 3 + 1] = rgb[pixel * 3 + 2] = v; };
    if (pfm) {
        if (scale == 0.0) Throw("\"{}\": invalid PFM scale", path);
        const bool little = scale < 0.0;
        std::vector<unsigned char> buf(n * 4);
        is.read((char *) buf.data(), (std::streamsize) buf.size());
        if ((size_t) is.gcount() != buf.size()) Throw("\"{}\": truncated image file ({} of {} bytes of pixel data)", path, (size_t) is.gcount(), buf.size());
        for (size_t k = 0; k < n; ++k) {
            const unsigned char *b = &buf[k * 4];
            const uint32_t bits = little ? (uint32_t) b[0] | (uint32_t) b[1] << 8 | (uint32_t) b[2] << 16 | (uint32_t) b[3] << 24
                                         : (uint32_t) b[3] | (uint32_t) b[2] << 8 | (uint32_t) b[1] << 16 | (uint32_t) b[0] << 24;
            float v; std::memcpy(&v, &bits, 4);
            const size_t px = k / channels, row = px / w, col = px % w;
            put(((size_t) h - 1 - row) * w + col, (int) (k % channels), v);      // the file's first row is the image's bottom row
        }
        return;
    }
    const long maxval = std::strtol(third.c_str(), nullptr, 10);
    if (maxval < 1 || maxval > 65535) Throw("\"{}\": invalid maxval {}", path, third);
    const size_t bps = maxval > 255 ? 2 : 1;
    std::vector<unsigned char> buf(n * bps);
    is.read((char *) buf.data(), (std::streamsize) buf.size());
    if ((size_t) is.gcount() != buf.size()) Throw("\"{}\": truncated image file ({} of {} bytes of pixel data)", path, (size_t) is.gcount(), buf.size());
    for (size_t k = 0; k < n; ++k) {
        const unsigned v = bps == 2 ? (unsigned) buf[k * 2] << 8 | buf[k * 2 + 1] : buf[k];      // (two-byte samples: most significant first)
        const double e = (double) v / (double) maxval;
        put(k / channels, (int) (k % channels), raw ? (float) e : srgb_to_linear(e));
    }
}

void write_exr(const std::string &path, int w, int h, const std::vector<std::string> &channels, const float *data) {
    std::ofstream os(path, std::ios::binary);
    if (!os) Throw("Could not open \"{}\" for writing", path);
    auto put32 = [&](uint32_t v) { os.write((const char *) &v, 4); };
    auto put64 = [&](uint64_t v) { os.write((const char *) &v, 8); };
    auto attr = [&](const char *name, const char *type, const std::string &payload) {
        os.write(name, std::strlen(name) + 1); os.write(type, std::strlen(type) + 1);
        put32((uint32_t) payload.size()); os.write(payload.data(), (std::streamsize) payload.size());
    };
    put32(20000630u); put32(2u);                           // magic, version 2, single-part scanline
    std::vector<size_t> order(channels.size());            // channels are stored alphabetically
    for (size_t i = 0; i < order.size(); ++i) order[i] = i;
    std::sort(order.begin(), order.end(), [&](size_t a, size_t b) { return channels[a] < channels[b]; });
    std::string ch;
    for (size_t i : order) {
        ch += channels[i]; ch += '\0';
        uint32_t v[4] = {2u /* FLOAT */, 0u, 1u, 1u};       // type, pLinear + reserved, xSampling, ySampling
        ch.append((const char *) v, 16);
    }
    ch += '\0';
    attr("channels", "chlist", ch);
    attr("compression", "compression", std::string(1, '\0'));
    int32_t box[4] = {0, 0, w - 1, h - 1};
    attr("dataWindow", "box2i", std::string((const char *) box, 16));
    attr("displayWindow", "box2i", std::string((const char *) box, 16));
    attr("lineOrder", "lineOrder", std::string(1, '\0'));
    float one = 1.f, zero2[2] = {0.f, 0.f};
    attr("pixelAspectRatio", "float", std::string((const char *) &one, 4));
    attr("screenWindowCenter", "v2f", std::string((const char *) zero2, 8));
    attr("screenWindowWidth", "float", std::string((const char *) &one, 4));
    os.put('\0');
    const size_t nc = channels.size();
    const uint64_t line_bytes = (uint64_t) w * nc * 4;
    uint64_t offset = (uint64_t) os.tellp() + (uint64_t) h * 8;
    for (int y = 0; y < h; ++y) { put64(offset); offset += 8 + line_bytes; }
    std::vector<float> row((size_t) w);
    for (int y = 0; y < h; ++y) {
        put32((uint32_t) y); put32((uint32_t) line_bytes);
        for (size_t i : order) {
            for (int x = 0; x < w; ++x) row[x] = data[((size_t) y * w + x) * nc + i];
            os.write((const char *) row.data(), (std::streamsize) w * 4);
        }
    }
}

}  // namespace misaki
