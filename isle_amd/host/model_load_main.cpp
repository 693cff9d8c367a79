// isle_amd/host/model_load_main.cpp — a model through its text and back, on the device and on the host, side by side: reads a raw
// float32 model (vocab x ncols, column-major), writes <base>.sparse / <base>.dense with FPSparseMatrixHip::write_model_text, loads each
// file with FPSparseMatrixHip::load_model_file and with the host parser of model_read.h, and writes what they hold as <base>.<format>.dev.f32
// and <base>.<format>.host.f32 (column-major), so that a test can hold the device loader to the C++ parser's own floats
// (tests/test_gpu_model_load_host_cpp.py).  stdout: "<format> <entries>" per format.
//   model_load_main <model.f32> <vocab> <ncols> <base>
#include "model_read.h"
#include "trainer_hip.h"

using namespace ISLE;

static void dump(const std::string& path, const std::vector<FPTYPE>& m) {
  std::ofstream f(path, std::ios::binary);
  f.write((const char*)m.data(), (std::streamsize)(m.size() * sizeof(FPTYPE)));
  if (!f) throw std::runtime_error("cannot write " + path);
}

int main(int argc, char** argv) {
  if (argc != 5) {
    std::cerr << "usage: model_load_main <model.f32> <vocab> <ncols> <base>\n";
    return 2;
  }
  const word_id_t vocab = atol(argv[2]);
  const doc_id_t ncols = atol(argv[3]);
  const std::string base = argv[4];
  try {
    std::vector<FPTYPE> model((size_t)vocab * ncols);
    std::ifstream in(argv[1], std::ios::binary);
    in.read((char*)model.data(), (std::streamsize)(model.size() * sizeof(FPTYPE)));
    if ((size_t)in.gcount() != model.size() * sizeof(FPTYPE)) throw std::runtime_error(std::string("short read on ") + argv[1]);
    FPSparseMatrixHip dev(vocab, 0);
    for (int format : {ISLE_TEXT_SPARSE, ISLE_TEXT_DENSE}) {
      const std::string name = format == ISLE_TEXT_SPARSE ? "sparse" : "dense", file = base + "." + name;
      dev.write_model_text(ISLE_MODEL_HOST, format, file, model.data(), vocab, ncols);
      const uint64_t n = dev.load_model_file(file, vocab, ncols, format);
      std::vector<FPTYPE> got, want;
      dev.get_loaded_model(got);
      const std::vector<char> text = model_read::read_file(file);
      if (format == ISLE_TEXT_SPARSE) {
        std::vector<FPTYPE> by_word;
        model_read::read_sparse_model(text.data(), text.size(), ncols, vocab, 1, by_word, nullptr);
        want.resize(by_word.size());
        for (word_id_t w = 0; w < vocab; ++w)
          for (doc_id_t t = 0; t < ncols; ++t) want[w + t * vocab] = by_word[w * ncols + t];
      } else {
        model_read::read_dense_model(text.data(), text.size(), ncols, vocab, want);
      }
      dump(file + ".dev.f32", got);
      dump(file + ".host.f32", want);
      std::cout << name << " " << n << std::endl;
    }
  } catch (const std::exception& e) {
    std::cerr << "model_load_main failed: " << e.what() << std::endl;
    return 1;
  }
  return 0;
}
