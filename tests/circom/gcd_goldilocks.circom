pragma circom 2.0.0;

// Euclid's algorithm as a witness hint: the loop runs a value-dependent number of times, so the function stays a run-time
// function (compiled with --prime goldilocks it runs in the 64-bit runtime's interpreter).
function gcd(a, b) {
    while (b != 0) {
        var t = a % b;
        a = b;
        b = t;
    }
    return a;
}

template Gcd() {
    signal input a;
    signal input b;
    signal output out;
    signal k;
    out <-- gcd(a, b);
    k <-- a \ out;          // integer division: gcd(0, 0) = 0 is a division by zero here
    k * out === a;
}

component main = Gcd();
