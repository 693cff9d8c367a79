// isle_amd/host/model_text_main.cpp — a model's two text forms by the host writers and by the device path, side by side: reads a raw
// float32 model (vocab x ncols, column-major) and writes <base>.host.sparse / <base>.host.dense with trainer_detail::write_dense_as_sparse /
// write_dense (trainer_hip.h) and <base>.dev.sparse / <base>.dev.dense with FPSparseMatrixHip::write_model_text(ISLE_MODEL_HOST, ...), so that a
// test can compare the device text with the C++ writer's own bytes (tests/test_gpu_model_text.py).  A model the device path refuses
// (an entry outside the writer's domain) leaves the .dev file empty and makes the exit status 3.  With [reps] every writer runs that many
// times and one line "<name> <median wall ms>" per file goes to stdout (tools/model_text_probe.py).
//   model_text_main <model.f32> <vocab> <ncols> <base> [reps]
#include "trainer_hip.h"

using namespace ISLE;

template <class F>
static void timed(const char* name, int reps, F&& f) {
  std::vector<double> ms;
  for (int i = 0; i < std::max(reps, 1); ++i) {
    const auto t0 = std::chrono::steady_clock::now();
    f();
    ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
  }
  std::sort(ms.begin(), ms.end());
  if (reps > 0) std::cout << name << " " << ms[ms.size() / 2] << std::endl;
}

int main(int argc, char** argv) {
  if (argc != 5 && argc != 6) {
    std::cerr << "usage: model_text_main <model.f32> <vocab> <ncols> <base> [reps]\n";
    return 2;
  }
  const int reps = argc == 6 ? atoi(argv[5]) : 0;
  const word_id_t vocab = atol(argv[2]);
  const doc_id_t ncols = atol(argv[3]);
  const std::string base = argv[4];
  try {
    std::vector<FPTYPE> model((size_t)vocab * ncols);
    std::ifstream in(argv[1], std::ios::binary);
    in.read((char*)model.data(), (std::streamsize)(model.size() * sizeof(FPTYPE)));
    if ((size_t)in.gcount() != model.size() * sizeof(FPTYPE)) throw std::runtime_error(std::string("short read on ") + argv[1]);
    timed("host.sparse", reps, [&] { trainer_detail::write_dense_as_sparse(base + ".host.sparse", model.data(), vocab, ncols); });
    timed("host.dense", reps, [&] { trainer_detail::write_dense(base + ".host.dense", model.data(), vocab, ncols); });
    FPSparseMatrixHip dev(vocab, 0);
    int status = 0;
    for (int format : {ISLE_TEXT_SPARSE, ISLE_TEXT_DENSE}) {
      const char* ext = format == ISLE_TEXT_SPARSE ? ".dev.sparse" : ".dev.dense";
      try {
        timed(ext + 1, reps, [&] { dev.write_model_text(ISLE_MODEL_HOST, format, base + ext, model.data(), vocab, ncols); });
      } catch (const std::exception& e) {
        std::cerr << "model_text_main: " << e.what() << std::endl;
        status = 3;
      }
    }
    return status;
  } catch (const std::exception& e) {
    std::cerr << "model_text_main failed: " << e.what() << std::endl;
    return 1;
  }
}
