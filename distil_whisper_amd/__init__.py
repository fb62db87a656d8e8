"""MI355X-native hot path of huggingface/distil-whisper (Whisper distillation step).  See DESIGN.md.

Public surface:
  ops_hip.HipOps                      ctypes binding of libdwamd.so (C ABI in include/dwamd.h); no CPU fallback
  engine.{WhisperDims, ParamStore, WhisperEngine}   flat parameter store + hand-written forward/backward
  distill.DistillationTrainer        teacher fwd + student fwd/bwd + RCCL all-reduce + fused clip/AdamW
  topk_distill.TeacherTopK           stored top-k teacher targets: a step without the teacher forward (also `from distil_whisper_amd import TeacherTopK`)
  modeling.{WhisperFeatureExtractor, WhisperForConditionalGeneration, WhisperForCausalLM}   reference-shaped drop-in classes
                                      (the last two are also importable from the package: `from distil_whisper_amd import ...`)
  collator.DataCollatorSpeechSeq2SeqWithPadding, student_init.student_from_teacher
"""
__version__ = "0.1.0"


def __getattr__(name):          # lazily: importing the package alone loads neither torch nor the library
    if name in ("WhisperForConditionalGeneration", "WhisperForCausalLM", "WhisperFeatureExtractor"):
        from . import modeling
        return getattr(modeling, name)
    if name == "TeacherTopK":
        from .topk_distill import TeacherTopK
        return TeacherTopK
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
