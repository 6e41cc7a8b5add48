// msd_keycodec.hpp -- order-preserving codes for signed and float keys ("Typed keys and indices").
//
// A key type is ordered through an unsigned CODE of the key's width: unsigned order of the codes is the ascending
// order of the keys, and the map between a key's bit pattern b and its code e is a bijection:
//
//   e = b ^ c0 ^ (sra(b, W-1) & c1)                     sra = arithmetic shift right, W = 32 or 64
//   b = t ^ (sra(t, W-1) & c1)   with t = e ^ c0        (c1 never has the top bit: b and t have the same top bit)
//
//   unsigned: c0 = 0,        c1 = 0                     the identity
//   signed:   c0 = sign bit, c1 = 0                     two's complement: flip the sign bit
//   float:    c0 = sign bit, c1 = all ones but the sign bit: a negative number has all its other bits flipped too
//
// The float order is IEEE-754 totalOrder on the bit patterns:
//   -NaN < -inf < ... < -denormal < -0 < +0 < +denormal < ... < +inf < +NaN
// (among NaNs of one sign: by payload).  Keys come back BIT-EXACT: NaN payloads and the sign of zero survive.  This
// differs from torch.topk / torch.sort only for NaNs with the sign bit set -- torch puts every NaN on top, here they
// lie below -inf -- and in that -0 and +0 are told apart (-0 first).
//
// The constants are run-time values (two words in a kernel's arguments), not a template policy: the select kernels
// get ONE typed instance per key width, whatever the key type.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MSD_HD __host__ __device__ __forceinline__
#else
#define MSD_HD inline
#endif

namespace msd {

// (the values of MSD_KEY_* in include/msd_radix_hip.h)
enum { kKeyU32 = 0, kKeyI32 = 1, kKeyF32 = 2, kKeyU64 = 3, kKeyI64 = 4, kKeyF64 = 5, kKeyTypes = 6 };

template <typename K> struct signed_of;
template <> struct signed_of<uint32_t> { typedef int32_t type; };
template <> struct signed_of<uint64_t> { typedef int64_t type; };

// A search direction is part of the constants for free: the search works on code ^ flip (msd_select.hpp), which is the code
// under { c0 ^ flip, c1 }.
// (Filter pass over 2^30 float32 keys, per-phase times of single runs: this form -- shift, AND, two XORs -- about 0.90 ms; a
// compare and a select per key 1.32 ms; (m & neg) | (~m & pos) with two precomputed constants, which the compiler turns into
// compare and select as well, 1.24 ms; plain unsigned keys 0.79 ms.  Every compare of a wave writes a scalar register pair,
// and the filter is short of those.)
template <typename K> struct KeyCodec {
	K c0, c1;
	typedef typename signed_of<K>::type S;
	// all ones where b has the top bit (>> of a negative signed value is an arithmetic shift in every compiler this builds with)
	static MSD_HD K sra(K b) { return (K)((S)b >> (sizeof(K) * 8 - 1)); }
	MSD_HD K enc(K b) const { return (K)(b ^ c0 ^ (sra(b) & c1)); }
	MSD_HD K dec(K e) const
	{
		const K t = (K)(e ^ c0);
		return (K)(t ^ (sra(t) & c1));
	}
	MSD_HD KeyCodec flipped(K flip) const { return KeyCodec{ (K)(c0 ^ flip), c1 }; }
};

constexpr int key_type_bytes(int key_type) { return key_type < kKeyU64 ? 4 : 8; }

// key_type: one of kKey* of K's width
template <typename K> MSD_HD KeyCodec<K> key_codec(int key_type)
{
	const K sign = (K)1 << (sizeof(K) * 8 - 1);
	const int kind = key_type % 3; // 0 unsigned, 1 signed, 2 float
	return KeyCodec<K>{ kind == 0 ? (K)0 : sign, kind == 2 ? (K)~sign : (K)0 };
}

} // namespace msd
